"""Group passes (ju_process_group; engine_passes.cpp "Group passes") -- needs an MI355X.

One frame for each of several runtimes in one call: the lead runs the flow net once over every member's frame, each
with its own runtime's history, then every member's warp, tower and tail.  The contract is byte equality with
ju_process on each runtime in list order.  Every member here has a TWIN -- a runtime built from the same bytes, driven
by ju_process with the same frames -- and outputs are compared byte for byte at every step, states at the end.
"""

import dataclasses
import threading

import numpy as np
import pytest

from helpers import M, small_config
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _device_frames(cfg, n, seed):
    torch, dev = _torch()
    frames = M.synthetic_frames(n, cfg.frame_height, cfg.frame_width, seed=seed, kind="noise")
    d_in = torch.from_numpy(frames).to(dev)
    torch.cuda.synchronize()
    return frames, d_in


def _device_outs(cfg, n):
    torch, dev = _torch()
    return torch.zeros((n, 4 * cfg.frame_height, 4 * cfg.frame_width, 4), dtype=torch.uint8, device=dev)


class Fleet:
    """`n` members and their twins, one device output buffer each."""

    def __init__(self, blob, dtype, cfg, n, twin_blob=None):
        self.cfg = cfg
        self.h, self.w = cfg.frame_height, cfg.frame_width
        self.members = [R.Runtime(blob, 0, dtype) for _ in range(n)]
        self.twins = [R.Runtime(blob if twin_blob is None else twin_blob, 0, dtype) for _ in range(n)]
        self.out = _device_outs(cfg, n)
        self.tw_out = _device_outs(cfg, n)

    def close(self):
        for rt in self.members + self.twins:
            rt.close()

    def img_in(self, rt, d):
        return rt.device_image(d.data_ptr(), self.w, self.h)

    def img_out(self, rt, d):
        return rt.device_image(d.data_ptr(), 4 * self.w, 4 * self.h)

    def group(self, idx, srcs):
        """A group call over members idx (srcs[k] = device frame of member idx[k]) and the twins' ju_process."""
        rts = [self.members[i] for i in idx]
        R.process_group(rts, [self.img_in(rt, s) for rt, s in zip(rts, srcs)],
                        [self.img_out(rt, self.out[i]) for rt, i in zip(rts, idx)])
        for i, s in zip(idx, srcs):
            self.twins[i].process(self.img_in(self.twins[i], s), self.img_out(self.twins[i], self.tw_out[i]))

    def plain(self, i, src):
        """ju_process on member i and its twin."""
        for rt, o in ((self.members[i], self.out), (self.twins[i], self.tw_out)):
            rt.process(self.img_in(rt, src), self.img_out(rt, o[i]))

    def assert_equal(self, idx, what=""):
        torch, _ = _torch()
        torch.cuda.synchronize()
        for i in idx:
            assert torch.equal(self.out[i], self.tw_out[i]), (what, i)

    def assert_states(self, idx=None):
        for i in (range(len(self.members)) if idx is None else idx):
            a, b = self.members[i], self.twins[i]
            if a.recurrent:
                assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), i
                assert np.array_equal(a.read_tensor("flow_in"), b.read_tensor("flow_in")), i


@pytest.mark.parametrize("preset,dtype", [("psp-quality", R.DTYPE_BF16), ("psp-fast", R.DTYPE_F16),
                                          ("ps2-quality", R.DTYPE_FP8), ("psp-quality-lrelu", R.DTYPE_BF16)])
def test_group_calls_give_the_bytes_of_ju_process(preset, dtype):
    """Groups of 2..8 of eight runtimes, the lead changing from call to call, members on different binding-set parities
    (some advanced by a plain ju_process first): every output at every step and every state at the end equal the
    twins'."""
    cfg = M.PRESETS[preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 12, seed=5)
    f = Fleet(blob, dtype, cfg, 8)
    try:
        for i in (1, 4, 6):
            f.plain(i, d_in[i])
        calls = [0] * 8
        for step, k in enumerate((2, 8, 5, 3, 8, 7, 4, 6)):
            idx = [(3 * step + j) % 8 for j in range(k)]
            f.group(idx, [d_in[(3 * i + step) % 12] for i in idx])
            f.assert_equal(idx, (step, k))
            for i in idx:
                calls[i] += 1
        f.assert_states()
        assert [rt.stat("group_frames") for rt in f.members] == calls, "the calls did not take group passes"
        assert all(rt.stat("group_frames") == 0 for rt in f.twins)
    finally:
        f.close()


def test_group_calls_mix_with_plain_calls_batches_and_resets():
    """One member also goes through ju_process, ju_process_batch and ju_reset between group calls: the next group call
    still equals the twins."""
    cfg = small_config()
    h, w = cfg.frame_height, cfg.frame_width
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 10, seed=9)
    f = Fleet(blob, R.DTYPE_F16, cfg, 3)
    batch_out = _device_outs(cfg, 3)
    tw_batch_out = _device_outs(cfg, 3)
    torch, _ = _torch()
    try:
        idx = [0, 1, 2]
        step = 0

        def group():
            nonlocal step
            f.group(idx, [d_in[(i + step) % 10] for i in idx])
            f.assert_equal(idx, step)
            step += 1

        group()
        f.plain(1, d_in[7])
        group()
        # a look-ahead pass on member 1; its twin takes the same frames one by one
        ins = [d_in[t] for t in (3, 4, 5)]
        f.members[1].process_batch([f.img_in(f.members[1], s) for s in ins],
                                   [f.img_out(f.members[1], batch_out[k]) for k in range(3)])
        for k, s in enumerate(ins):
            f.twins[1].process(f.img_in(f.twins[1], s), f.img_out(f.twins[1], tw_batch_out[k]))
        torch.cuda.synchronize()
        assert torch.equal(batch_out, tw_batch_out)
        assert f.members[1].stat("lookahead_frames") == 3
        group()
        f.members[1].reset()
        f.twins[1].reset()
        group()
        f.members[0].reset()  # (the lead)
        f.twins[0].reset()
        group()
        f.plain(0, d_in[2])
        group()
        f.assert_states()
        assert f.members[1].stat("group_frames") == step
    finally:
        f.close()


def test_host_padded_bottom_up_and_mixed_frames():
    """Host frames, padded strides, bottom-up (negative) strides, host and device frames in one call.  A member whose
    device output is off the kernels' 8-byte alignment cannot ride in the pass: it runs on its own, same bytes."""
    torch, dev = _torch()
    cfg = small_config()
    h, w = cfg.frame_height, cfg.frame_width
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    frames, d_in = _device_frames(cfg, 6, seed=13)
    n = 6
    members = [R.Runtime(blob, 0, R.DTYPE_BF16) for _ in range(n)]
    twins = [R.Runtime(blob, 0, R.DTYPE_BF16) for _ in range(n)]
    pad = 64
    try:
        # host outputs, one bottom-up; device input with padded rows, device bottom-up in / out, a misaligned output
        host_out = [np.zeros((4 * h, 4 * w, 4), np.uint8) for _ in range(n)]
        padded_in = torch.zeros((h, w * 4 + pad), dtype=torch.uint8, device=dev)
        dev_out = torch.zeros((n, 4 * h, 4 * w * 4 + pad), dtype=torch.uint8, device=dev)
        misaligned = torch.zeros(4 * h * 4 * w * 4 + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def images(rt, k, t):
            src = frames[(k + t) % 6]
            if k == 0:   # host in, host out
                return R.host_image(src), R.host_image(host_out[0])
            if k == 1:   # padded device in, padded device out
                return (rt.device_image(padded_in.data_ptr(), w, h, w * 4 + pad),
                        rt.device_image(dev_out[1].data_ptr(), 4 * w, 4 * h, 4 * w * 4 + pad))
            if k == 2:   # host bottom-up in and out
                flipped = np.ascontiguousarray(src[::-1])[::-1]
                images.keep.append(flipped)
                return R.host_image(flipped), R.host_image(host_out[2][::-1])
            if k == 3:   # device bottom-up in and out
                row = w * 4
                last = d_in[(k + t) % 6].view(h, row)
                return (rt.device_image(last[h - 1].data_ptr(), w, h, -row),
                        rt.device_image(dev_out[3][4 * h - 1].data_ptr(), 4 * w, 4 * h, -(4 * w * 4 + pad)))
            if k == 4:   # device in, host out
                return rt.device_image(d_in[(k + t) % 6].data_ptr(), w, h), R.host_image(host_out[4])
            # device output 4 bytes off the 8-byte alignment a pass needs
            return rt.device_image(d_in[(k + t) % 6].data_ptr(), w, h), rt.device_image(misaligned.data_ptr() + 4, 4 * w, 4 * h)
        images.keep = []

        def snapshot(k):
            torch.cuda.synchronize()
            if k in (0, 2, 4):
                return host_out[k].copy()
            if k in (1, 3):
                return dev_out[k].cpu().numpy().copy()
            return misaligned.cpu().numpy().copy()

        for t in range(3):
            padded_in[:, : w * 4] = d_in[(1 + t) % 6].view(h, w * 4)
            torch.cuda.synchronize()
            pairs = [images(members[k], k, t) for k in range(n)]
            R.process_group(members, [p[0] for p in pairs], [p[1] for p in pairs])
            got = [snapshot(k) for k in range(n)]
            for k in range(n):
                tin, tout = images(twins[k], k, t)
                twins[k].process(tin, tout)
                assert np.array_equal(snapshot(k), got[k]), (t, k)
        for k in range(n):
            assert np.array_equal(members[k].read_tensor("state"), twins[k].read_tensor("state")), k
        assert [m.stat("group_frames") for m in members] == [3, 3, 3, 3, 3, 0]
    finally:
        for rt in members + twins:
            rt.close()


def test_long_calls_split_into_passes_and_one_member_is_ju_process():
    """count above the lead's cap: consecutive passes (8 + 3, and with a cap of 3: 3 + 3 + 1, the last member as a plain
    call).  count == 1 is ju_process."""
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 11, seed=17)
    f = Fleet(blob, R.DTYPE_F16, cfg, 11)
    try:
        idx = list(range(11))
        f.group(idx, [d_in[i] for i in idx])
        f.assert_equal(idx, "11")
        assert all(rt.stat("group_frames") == 1 for rt in f.members)
        f.members[0].set_lookahead(3)
        idx7 = list(range(7))
        f.group(idx7, [d_in[(i + 1) % 11] for i in idx7])
        f.assert_equal(idx7, "7 of cap 3")
        assert [f.members[i].stat("group_frames") for i in idx7] == [2, 2, 2, 2, 2, 2, 1]
        f.group([5], [d_in[3]])
        f.assert_equal([5], "1")
        assert f.members[5].stat("group_frames") == 2
        f.assert_states()
        # count == 0: nothing happens
        R.process_group([], [], [])
    finally:
        f.close()


def test_a_pass_whose_resident_tower_times_out_is_run_again_member_by_member():
    """The simulated expiry of the resident tower's bounded wait (the test hook makes the tower report it; no GPU fault)
    inside a group pass: the engine falls back to the per-block kernels and runs the same frames again, member by
    member -- no error, and the bytes of twins that met the same switch at the same frame."""
    cfg = M.PRESETS["psp-fast"]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 8, seed=41)
    lib = R.load_library()
    f = Fleet(blob, R.DTYPE_BF16, cfg, 3)
    try:
        assert all(rt.stat("resident_tower") == 1 for rt in f.members)
        idx = [0, 1, 2]
        f.plain(2, d_in[7])
        for step in range(5):
            srcs = [d_in[(i + step) % 8] for i in idx]
            if step == 2:
                rts = f.members
                lib.ju_debug_set(b"resident_fault", 1)
                try:
                    R.process_group(rts, [f.img_in(rt, s) for rt, s in zip(rts, srcs)],
                                    [f.img_out(rt, f.out[i]) for rt, i in zip(rts, idx)])
                    for i, s in zip(idx, srcs):
                        f.twins[i].process(f.img_in(f.twins[i], s), f.img_out(f.twins[i], f.tw_out[i]))
                finally:
                    lib.ju_debug_set(b"resident_fault", 0)
                f.assert_equal(idx, "fault")
                continue
            f.group(idx, srcs)
            f.assert_equal(idx, step)
        f.assert_states()
        assert all(rt.stat("fallbacks") == 1 for rt in f.members + f.twins)
        assert all(rt.stat("group_frames") == 4 for rt in f.members)
    finally:
        f.close()


@pytest.mark.parametrize("variant", ["flow-resnet", "brightness", "generic-flow"])
def test_models_without_a_batched_flow_plan_go_member_by_member(variant, monkeypatch):
    if variant == "generic-flow":
        monkeypatch.setenv("JU_FLOW_CONV", "generic")
        cfg = small_config()
    elif variant == "brightness":
        cfg = small_config(normalize_brightness=True)
    else:
        cfg = dataclasses.replace(M.PRESETS["psp-quality-flowres"], frame_height=64, frame_width=96)
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 6, seed=3)
    f = Fleet(blob, R.DTYPE_F16, cfg, 3)
    try:
        idx = [0, 1, 2]
        for step in range(3):
            f.group(idx, [d_in[(i + step) % 6] for i in idx])
            f.assert_equal(idx, (variant, step))
        f.assert_states()
        assert all(rt.stat("group_frames") == 0 for rt in f.members), variant
    finally:
        f.close()


def test_an_output_over_another_members_input_goes_member_by_member_in_list_order():
    torch, dev = _torch()
    cfg = small_config()
    h, w = cfg.frame_height, cfg.frame_width
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 4, seed=29)
    f = Fleet(blob, R.DTYPE_BF16, cfg, 3)
    arena = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    tw_arena = torch.zeros_like(arena)
    try:
        for step in range(2):
            arena.view(-1)[: h * w * 4] = d_in[step].view(-1)
            tw_arena.view(-1)[: h * w * 4] = d_in[step].view(-1)
            torch.cuda.synchronize()
            # member 0 reads the arena's head; member 1 writes the arena; member 2 is unrelated
            m, t = f.members, f.twins
            R.process_group(m, [m[0].device_image(arena.data_ptr(), w, h), f.img_in(m[1], d_in[2]), f.img_in(m[2], d_in[3])],
                            [f.img_out(m[0], f.out[0]), f.img_out(m[1], arena), f.img_out(m[2], f.out[2])])
            t[0].process(t[0].device_image(tw_arena.data_ptr(), w, h), f.img_out(t[0], f.tw_out[0]))
            t[1].process(f.img_in(t[1], d_in[2]), f.img_out(t[1], tw_arena))
            t[2].process(f.img_in(t[2], d_in[3]), f.img_out(t[2], f.tw_out[2]))
            f.assert_equal([0, 2], step)
            assert torch.equal(arena, tw_arena), step
        f.assert_states()
        assert all(rt.stat("group_frames") == 0 for rt in f.members)
    finally:
        f.close()


@pytest.mark.parametrize("variant", ["temporal", "noflow"])
def test_temporal_filter_and_flow_free_models_ride_in_the_passes(variant):
    """The temporal output filter (each member keeps its own accumulators) and a flow-free model (the pass is the
    members' generator programs) go as group passes, same bytes."""
    if variant == "temporal":
        cfg = dataclasses.replace(M.PRESETS["psp-fast"], temporal_strength=0.6, temporal_window=3)
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    else:
        base = M.PRESETS["psp-quality"]
        cfg, wts = M.remove_flow(base, M.make_seeded_weights(base))  # psp-quality-noflow
        blob = M.serialize(cfg, wts)
    _, d_in = _device_frames(cfg, 6, seed=31)
    f = Fleet(blob, R.DTYPE_F16, cfg, 4)
    try:
        idx = [0, 1, 2, 3]
        f.plain(1, d_in[5])
        for step in range(4):
            sub = idx if step % 2 == 0 else [2, 0, 3]
            f.group(sub, [d_in[(i + step) % 6] for i in sub])
            f.assert_equal(sub, (variant, step))
        f.assert_states()
        assert all(rt.stat("group_frames") > 0 for rt in f.members), variant
    finally:
        f.close()


def test_refused_calls_change_nothing():
    """NULL arguments, a runtime twice, members of other weights or another dtype, one wrong-sized frame (also a
    graphics resource of a wrong declared width): each JU_ERR_INVALID_ARGUMENT, and every member's next frame still equals its twin's."""
    torch, dev = _torch()
    cfg = small_config()
    h, w = cfg.frame_height, cfg.frame_width
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    other = M.serialize(cfg, M.make_seeded_weights(cfg, seed=7))
    _, d_in = _device_frames(cfg, 6, seed=37)
    lib = R.load_library()
    f = Fleet(blob, R.DTYPE_BF16, cfg, 3)
    stranger = R.Runtime(other, 0, R.DTYPE_BF16)
    f16 = R.Runtime(blob, 0, R.DTYPE_F16)
    small = torch.zeros((h, w - 2, 4), dtype=torch.uint8, device=dev)
    try:
        idx = [0, 1, 2]
        f.group(idx, [d_in[i] for i in idx])
        m = f.members

        def call(rts, ins=None, outs=None, count=None):
            n = len(rts)
            hs = (R.C.c_void_p * max(n, 1))(*[rt._h.value for rt in rts])
            ins = ins or [f.img_in(rt, d_in[3]) for rt in rts]
            outs = outs or [f.img_out(rt, f.out[k % 3]) for k, rt in enumerate(rts)]
            a, b = (R.JuImage * n)(*ins), (R.JuImage * n)(*outs)
            return lib.ju_process_group(hs, a, b, n if count is None else count)

        n3 = (R.JuImage * 3)()
        hs3 = (R.C.c_void_p * 3)(*[rt._h.value for rt in m])
        assert lib.ju_process_group(None, n3, n3, 3) == JU_ERR_INVALID_ARGUMENT
        assert lib.ju_process_group(hs3, None, n3, 3) == JU_ERR_INVALID_ARGUMENT
        assert lib.ju_process_group(hs3, n3, None, 3) == JU_ERR_INVALID_ARGUMENT
        assert call(m, count=-1) == JU_ERR_INVALID_ARGUMENT
        assert lib.ju_process_group((R.C.c_void_p * 2)(m[0]._h.value, None), n3, n3, 2) == JU_ERR_INVALID_ARGUMENT
        assert call([m[0], m[1], m[0]]) == JU_ERR_INVALID_ARGUMENT
        assert b"twice" in lib.ju_last_error()
        assert call([m[0], stranger, m[2]]) == JU_ERR_INVALID_ARGUMENT
        assert call([m[0], m[1], f16]) == JU_ERR_INVALID_ARGUMENT
        assert b"does not match" in lib.ju_last_error()
        bad_in = [f.img_in(m[0], d_in[3]), m[1].device_image(small.data_ptr(), w - 2, h), f.img_in(m[2], d_in[3])]
        assert call(m, ins=bad_in) == JU_ERR_INVALID_ARGUMENT
        bad_out = [f.img_out(rt, f.out[k]) for k, rt in enumerate(m)]
        bad_out[2] = m[2].device_image(f.out[2].data_ptr(), 4 * w, 4 * h - 1)
        assert call(m, outs=bad_out) == JU_ERR_INVALID_ARGUMENT
        bad_stride = [f.img_out(rt, f.out[k]) for k, rt in enumerate(m)]
        bad_stride[1] = m[1].device_image(f.out[1].data_ptr(), 4 * w, 4 * h, 4 * w)
        assert call(m, outs=bad_stride) == JU_ERR_INVALID_ARGUMENT
        unknown = [f.img_in(rt, d_in[3]) for rt in m]
        unknown[1].location = 7
        assert call(m, ins=unknown) == JU_ERR_INVALID_ARGUMENT
        # a texture whose DECLARED width is wrong, among members whose frames are fine: refused before any member runs
        assert lib.ju_debug_fake_gl_texture(31, small.data_ptr(), (w - 2) * 4, w - 2, h, 4) == 0
        try:
            bad_gl = R.gl_image(31, output=False)
            assert (bad_gl.location, bad_gl.width) == (R.LOC_GRAPHICS_RESOURCE, w - 2)
            assert call(m, ins=[f.img_in(m[0], d_in[3]), bad_gl, f.img_in(m[2], d_in[3])]) == JU_ERR_INVALID_ARGUMENT
            R.release_gl_image(bad_gl)
        finally:
            lib.ju_debug_fake_gl_texture(0, None, 0, 0, 0, 0)
        with pytest.raises(R.JoshUpscaleError):
            R.process_group([m[0], stranger], [f.img_in(m[0], d_in[1]), f.img_in(stranger, d_in[1])],
                            [f.img_out(m[0], f.out[0]), f.img_out(stranger, f.out[1])])
        assert all(rt.stat("group_frames") == 1 for rt in m)
        for step in range(2):
            f.group(idx, [d_in[(i + 4 + step) % 6] for i in idx])
            f.assert_equal(idx, step)
        f.assert_states()
    finally:
        f.close()
        stranger.close()
        f16.close()


def test_pending_enqueued_work_and_a_concurrent_runtime_are_ordered():
    """A member with a ju_enqueue outstanding when the group call is made comes out right; a third runtime driven by
    ju_process from another thread during the group calls neither hangs nor changes a byte."""
    torch, dev = _torch()
    cfg = M.PRESETS["psp-quality"]
    h, w = cfg.frame_height, cfg.frame_width
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    _, d_in = _device_frames(cfg, 8, seed=43)
    f = Fleet(blob, R.DTYPE_BF16, cfg, 3)
    third, third_twin = R.Runtime(blob, 0, R.DTYPE_BF16), R.Runtime(blob, 0, R.DTYPE_BF16)
    side_out = _device_outs(cfg, 2)
    n_third = 24
    third_out = _device_outs(cfg, n_third)
    try:
        idx = [0, 1, 2]
        for step in range(3):
            # member 1 (and its twin) get one frame through ju_enqueue, not waited for
            for rt, o in ((f.members[1], side_out[0]), (f.twins[1], side_out[1])):
                rt.enqueue(f.img_in(rt, d_in[(step + 5) % 8]), f.img_out(rt, o))
            f.twins[1].synchronize()
            f.group(idx, [d_in[(i + step) % 8] for i in idx])
            f.members[1].synchronize()
            f.assert_equal(idx, step)
            torch.cuda.synchronize()
            assert torch.equal(side_out[0], side_out[1]), step

        errors = []

        def drive():
            try:
                for t in range(n_third):
                    third.process(third.device_image(d_in[t % 8].data_ptr(), w, h),
                                  third.device_image(third_out[t].data_ptr(), 4 * w, 4 * h))
            except Exception as e:  # pragma: no cover - reported below
                errors.append(e)

        th = threading.Thread(target=drive)
        th.start()
        for step in range(3, 9):
            f.group(idx, [d_in[(i + step) % 8] for i in idx])
            f.assert_equal(idx, step)
        th.join(timeout=120)
        assert not th.is_alive(), "the concurrent runtime hung"
        assert not errors, errors
        want = _device_outs(cfg, 1)
        for t in range(n_third):
            third_twin.process(third_twin.device_image(d_in[t % 8].data_ptr(), w, h),
                               third_twin.device_image(want[0].data_ptr(), 4 * w, 4 * h))
            torch.cuda.synchronize()
            assert torch.equal(want[0], third_out[t]), t
        f.assert_states()
        assert all(rt.stat("group_frames") == 9 for rt in f.members)
    finally:
        f.close()
        third.close()
        third_twin.close()
