"""Group passes on frames of any format (ju_process_group_frames; engine_passes.cpp "Group passes"): every plane of every
member equals what ju_process_frame twins write, byte for byte, with the state and the frame history; BGRX-only calls are
ju_process_group; the overlap rule on planes; a staged member beside the pass; refused calls change nothing; and the scene
detector of host NV12 members inside the pass."""

import numpy as np
import pytest

import scene_reference as S
import test_gpu_packed10 as PK
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_packed10 import Side, Spec
from test_gpu_scene import known
from test_gpu_source import same_state
from test_gpu_yuv import torch_dev
from test_gpu_yuv10 import NV12, decoded, source
from test_group_frames_cpu import ROTATED_CUTS, rotated

pytestmark = pytest.mark.gpu

THR = S.KNOWN_THRESHOLD
CS = R.CS_BT709_LIMITED
H, W = 30, 48
BGRX, I420, P010, YUY2, BGR24, BGRX64, RGBPH, V210, Y410 = 0, 1, 3, 16, 32, 35, 39, 48, 50
DTYPE = R.DTYPE_BF16

# member: input -> output, mixed per member and side, host and device planes, one member bottom-up on both sides
SPECS = [Spec(NV12, "host", "plain", P010, "host", "padded"),
         Spec(I420, "device", "padded", NV12, "device", "plain"),
         Spec(YUY2, "host", "padded", Y410, "device", "plain"),
         Spec(V210, "device", "bottom-up", BGRX64, "host", "bottom-up"),
         Spec(BGRX, "device", "plain", RGBPH, "device", "padded"),
         Spec(BGR24, "host", "plain", BGRX, "host", "plain")]


def blob_of(seed=None):
    cfg = small_config()
    return M.serialize(cfg, M.make_seeded_weights(cfg) if seed is None else M.make_seeded_weights(cfg, seed=seed))


def clips(members, ticks):
    """A clip of its own per member: their states differ on every tick."""
    return [M.synthetic_frames(ticks, H, W, seed=31 + k, kind="smooth") for k in range(members)]


def twin_planes(blob, frames, spec, setup=None):
    """What ju_process_frame writes for one member's frames on plain host planes; + its state and history."""
    want = []
    with R.Runtime(blob, 0, DTYPE) as rt:
        if setup:
            setup(rt)
        ow, oh = rt.frame_output_size()
        for f in frames:
            pout = PK.blank(spec.fout, oh, ow)
            pin = PK.source(f, spec.fin, spec.cin)                # (kept alive: the frame holds raw pointers)
            rt.process_frame(PK.host(spec.fin, pin, W, spec.cin), PK.host(spec.fout, pout, ow, spec.cout))
            want.append(pout)
        tensors = (rt.read_tensor("state").copy(), rt.read_tensor("flow_in").copy())
    return want, tensors


def sides(frames_now, specs, out_sizes=None):
    ins = [Side(s.fin, s.cin, s.lin, s.layin, PK.source(f, s.fin, s.cin), W, H) for f, s in zip(frames_now, specs)]
    sizes = out_sizes or [(4 * W, 4 * H)] * len(specs)
    outs = [Side(s.fout, s.cout, s.lout, s.layout, PK.blank(s.fout, oh, ow), ow, oh) for s, (ow, oh) in zip(specs, sizes)]
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def same_tensors(rt, pair):
    return np.array_equal(rt.read_tensor("state"), pair[0]) and np.array_equal(rt.read_tensor("flow_in"), pair[1])


def open_all(blob, n):
    return [R.Runtime(blob, 0, DTYPE) for _ in range(n)]


def close_all(rts):
    for rt in rts:
        rt.close()


# ---- 1. equality with ju_process_frame twins -----------------------------------------------------------------------------------
def test_mixed_formats_and_locations_equal_the_per_frame_twins():
    blob, ticks = blob_of(), 5
    clip = clips(len(SPECS), ticks)
    twins = [twin_planes(blob, clip[k], s) for k, s in enumerate(SPECS)]
    # "from that member's own state": members 0 (P010) and 2 (Y410) carry 10-bit luma of the same colour space -- encoded
    # from one state the two would agree; fed different clips they must not
    for t in range(ticks):
        y_p010 = twins[0][0][t][0] >> 6
        y_y410 = (twins[2][0][t][0] >> 10) & 1023
        assert y_p010.shape == y_y410.shape and not np.array_equal(y_p010, y_y410), t
    rts = open_all(blob, len(SPECS))
    try:
        assert all(rt.stat("hbd_from_state") == 1 for rt in rts)
        for t in range(ticks):
            ins, outs = sides([clip[k][t] for k in range(len(SPECS))], SPECS)
            R.process_group_frames(rts, [x.frame for x in ins], [x.frame for x in outs])
            for k in range(len(SPECS)):
                outs[k].check(twins[k][0][t])                     # every plane, and the guard bytes around device planes
                ins[k].check([p._rows(p.host) for p in ins[k].planes])
        for k, rt in enumerate(rts):
            assert same_tensors(rt, twins[k][1]), k
            assert rt.stat("group_frames") == ticks and rt.stat("group_yuv_frames") == ticks, k
            assert rt.stat("fallbacks") == 0 and rt.stat("lookahead_frames") == 0
    finally:
        close_all(rts)


# ---- 2. BGRX frames only ---------------------------------------------------------------------------------------------------------
def test_bgrx_frames_only_behave_as_process_group():
    torch, dev = torch_dev()
    blob, n, ticks = blob_of(), 3, 3
    clip = clips(n, ticks)
    d_in = torch.from_numpy(np.stack(clip)).to(dev)
    d_out = torch.zeros((2, n, 4 * H, 4 * W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    a, b = open_all(blob, n), open_all(blob, n)
    try:
        for t in range(ticks):
            R.process_group_frames(a, [R.device_frame(BGRX, W, H, [d_in[k][t]]) for k in range(n)],
                                   [R.device_frame(BGRX, 4 * W, 4 * H, [d_out[0][k]]) for k in range(n)])
            R.process_group(b, [b[k].device_image(d_in[k][t].data_ptr(), W, H) for k in range(n)],
                            [b[k].device_image(d_out[1][k].data_ptr(), 4 * W, 4 * H) for k in range(n)])
            got = d_out.cpu().numpy()
            assert np.array_equal(got[0], got[1]) and got[0].any(), t
        for x, y in zip(a, b):
            assert same_state(x, y)
            for key in ("group_frames", "group_yuv_frames", "graph_replays", "eager_runs", "lookahead_frames"):
                assert x.stat(key) == y.stat(key), key
            assert x.stat("group_frames") == ticks and x.stat("group_yuv_frames") == 0
    finally:
        close_all(a + b)


# ---- 3. an output plane over another member's input plane ------------------------------------------------------------------------
def test_an_output_plane_over_another_members_input_plane_runs_in_list_order():
    torch, dev = torch_dev()
    blob, ticks = blob_of(), 2
    clip = clips(2, ticks)

    def buffers():
        out1 = torch.zeros(4 * H * 4 * W * 4, dtype=torch.uint8, device=dev)     # member 1's BGRX output ...
        uv = torch.zeros(H // 2 * W, dtype=torch.uint8, device=dev)
        out0 = torch.zeros((4 * H, 4 * W, 4), dtype=torch.uint8, device=dev)
        in1 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        frames_in = [R.device_frame(NV12, W, H, [out1, uv], colorspace=CS),      # ... holds member 0's luma plane
                     R.device_frame(BGRX, W, H, [in1])]
        frames_out = [R.device_frame(BGRX, 4 * W, 4 * H, [out0]), R.device_frame(BGRX, 4 * W, 4 * H, [out1])]
        return out1, uv, out0, in1, frames_in, frames_out

    def load(bufs, t):
        y, uvp = source(clip[0][t], NV12, CS)
        bufs[0][:H * W] = torch.from_numpy(np.ascontiguousarray(y).reshape(-1)).to(dev)
        bufs[1][...] = torch.from_numpy(np.ascontiguousarray(uvp).reshape(-1)).to(dev)
        bufs[3][...] = torch.from_numpy(clip[1][t]).to(dev)
        torch.cuda.synchronize()

    a, b = open_all(blob, 2), open_all(blob, 2)
    ga, gb = buffers(), buffers()
    try:
        for t in range(ticks):
            load(ga, t)
            load(gb, t)
            R.process_group_frames(a, ga[4], ga[5])
            for k in range(2):                                    # list order: member 0 reads its luma before member 1 writes
                b[k].process_frame(gb[4][k], gb[5][k])
            for k in (0, 2):
                assert np.array_equal(ga[k].cpu().numpy(), gb[k].cpu().numpy()) and ga[k].any(), (t, k)
        for x, y in zip(a, b):
            assert same_state(x, y) and x.stat("group_frames") == 0 and x.stat("group_yuv_frames") == 0
    finally:
        close_all(a + b)


# ---- 4. a member under an output size ---------------------------------------------------------------------------------------------
def test_a_member_under_an_output_size_runs_on_its_own_beside_the_pass():
    blob, ticks = blob_of(), 3
    specs = [SPECS[0], Spec(NV12, "host", "plain", NV12, "device", "padded"), SPECS[4]]
    clip = clips(3, ticks)
    small = (96, 60)
    setups = [None, lambda rt: rt.set_output_size(*small), None]
    twins = [twin_planes(blob, clip[k], s, setups[k]) for k, s in enumerate(specs)]
    rts = open_all(blob, 3)
    try:
        rts[1].set_output_size(*small)
        for t in range(ticks):
            ins, outs = sides([clip[k][t] for k in range(3)], specs, [(4 * W, 4 * H), small, (4 * W, 4 * H)])
            R.process_group_frames(rts, [x.frame for x in ins], [x.frame for x in outs])
            for k in range(3):
                outs[k].check(twins[k][0][t])
        for k, rt in enumerate(rts):
            assert same_tensors(rt, twins[k][1]), k
        assert [rt.stat("group_frames") for rt in rts] == [ticks, 0, ticks]
        assert [rt.stat("source_stage_frames") for rt in rts] == [0, ticks, 0]
    finally:
        close_all(rts)


# ---- 5. refused calls change nothing ------------------------------------------------------------------------------------------------
STAT_KEYS = ("group_frames", "group_yuv_frames", "scene_group_frames", "scene_detector_runs", "scene_frames", "scene_cuts",
             "graph_replays", "eager_runs", "lookahead_frames", "fallbacks")


def snapshot(rts):
    return [(rt.read_tensor("state").copy(), rt.read_tensor("flow_in").copy(), rt.scene_info(), [rt.stat(k) for k in STAT_KEYS])
            for rt in rts]


def same_snapshot(x, y):
    return all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[2] == q[2] and p[3] == q[3] for p, q in zip(x, y))


def test_refused_calls_change_nothing():
    blob, n = blob_of(), 5
    clip = clips(n, 3)
    rts = open_all(blob, n)
    try:
        with R.Runtime(blob_of(seed=77), 0, DTYPE) as other:
            for rt in rts:
                rt.set_scene_detect(R.SCENE_RESET, THR)
                rt.set_scene_group(1)

            def frames(t):
                pin = [source(clip[k][t], NV12, CS) for k in range(n)]
                pout = [[np.zeros((4 * H, 4 * W), np.uint8), np.zeros((2 * H, 4 * W), np.uint8)] for _ in range(n)]
                return pin, pout, [R.host_frame(NV12, p, CS) for p in pin], [R.host_frame(NV12, p, CS) for p in pout]

            for t in range(2):
                keep = frames(t)
                R.process_group_frames(rts, keep[2], keep[3])
            before = snapshot(rts)
            assert all(s[3][0] == 2 and s[3][2] == 2 for s in before)

            def refused(members, ins, outs, words):
                with pytest.raises(R.JoshUpscaleError) as err:
                    R.process_group_frames(members, ins, outs)
                assert all(w in str(err.value) for w in words), str(err.value)
                assert same_snapshot(snapshot(rts), before), words
                assert all(not p.any() for planes in keep[1] for p in planes)      # nothing was written

            keep = frames(2)
            _, _, ins, outs = keep
            odd = list(ins)
            odd[3] = R._frame(NV12, CS, R.LOC_CPU, W, H + 1, [p.ctypes.data for p in keep[0][3]], [W, W])
            refused(rts, odd, outs, ["ju_process_group_frames", "member 3", "even"])
            null = list(outs)
            null[2] = R._frame(NV12, CS, R.LOC_CPU, 4 * W, 4 * H, [keep[1][2][0].ctypes.data, None], [4 * W, 4 * W])
            refused(rts, ins, null, ["member 2", "plane 1 is NULL"])
            unknown = list(ins)
            unknown[4] = R._frame(99, CS, R.LOC_CPU, W, H, [p.ctypes.data for p in keep[0][4]], [W, W])
            refused(rts, unknown, outs, ["member 4", "unknown format"])
            refused([rts[0], rts[1], rts[0], rts[3], rts[4]], ins, outs, ["runtime 2 appears twice"])
            refused([rts[0], other, rts[2], rts[3], rts[4]], ins, outs, ["runtime 1 does not match"])
            # and the same frames are taken once nothing is wrong with them
            R.process_group_frames(rts, ins, outs)
            assert all(rt.stat("group_frames") == 3 for rt in rts) and all(p.any() for planes in keep[1] for p in planes)
    finally:
        close_all(rts)


# ---- 6. the detector of host NV12 members inside the pass ----------------------------------------------------------------------------
def test_the_detector_of_host_nv12_members_sees_the_decoded_frames():
    blob, clip, _ = known()
    n = 4
    planes = [[source(f, NV12, CS) for f in rotated(clip, k)] for k in range(n)]
    want = [S.run([decoded(NV12, CS, p) for p in planes[k]], THR) for k in range(n)]
    assert [S.cuts(w) for w in want] == [ROTATED_CUTS[k] for k in range(n)]
    rts = open_all(blob, n)
    twins = open_all(blob, n)
    try:
        for rt in rts + twins:
            rt.set_scene_detect(R.SCENE_RESET, THR)
        for rt in rts:
            rt.set_scene_group(1)
        for t in range(13):
            got = [[np.zeros((4 * H, 4 * W), np.uint8), np.zeros((2 * H, 4 * W), np.uint8)] for _ in range(n)]
            exp = [[np.zeros((4 * H, 4 * W), np.uint8), np.zeros((2 * H, 4 * W), np.uint8)] for _ in range(n)]
            R.process_group_frames(rts, [R.host_frame(NV12, planes[k][t], CS) for k in range(n)],
                                   [R.host_frame(NV12, g, CS) for g in got])
            for k in range(n):
                twins[k].process_frame(R.host_frame(NV12, planes[k][t], CS), R.host_frame(NV12, exp[k], CS))
                assert all(np.array_equal(g, e) for g, e in zip(got[k], exp[k])), (t, k)
        for k, rt in enumerate(rts):
            assert rt.scene_info() == want[k] == twins[k].scene_info(), k
            assert same_state(rt, twins[k]), k
            assert rt.stat("scene_group_frames") == rt.stat("group_frames") == rt.stat("group_yuv_frames") == 13, k
            assert rt.stat("scene_detector_runs") == 13
    finally:
        close_all(rts + twins)
