"""Scaled and masked members inside group passes (ju_set_stage_group; docs/source_stage.md and docs/output_stage.md, "Group
passes"): the members kernel alone against the numpy definition and the single-frame kernel, byte for byte; the sized decode
launch alone against the launch of one size; group passes against twin runtimes with the same settings fed through
ju_process_frame -- every output plane with its guards, the state, the frame history, the detector's records and the stats;
other leads, models and dtypes, the detector, the re-run and a call longer than the lead's cap; settings changed and a
member destroyed between calls; the refusals and the routing."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import scale_filter_reference as F
import test_gpu_packed10 as PK
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_packed10 import Y210
from test_gpu_source import LAYOUTS, make_mask
from test_gpu_stage_passes import Setup, Side, Spec, blob_of, same_as, snapshot
from test_gpu_yuv import DevPlane, torch_dev

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
BGRX, NV12, P010, YUY2, V210 = R.FMT_BGRX, R.FMT_NV12, R.FMT_P010, R.FMT_YUY2, R.FMT_V210
SRC, SRC_ODD = (48, 72), (34, 50)        # (h, w) for the 30 x 48 model
DTYPE = R.DTYPE_BF16


# ---- 1. the members kernel alone ----------------------------------------------------------------------------------------
MEMBER_SIZES = [(30, 46), (17, 23), (8, 12), (16, 24), (4, 6)]   # reducing, odd, halving, passing through, enlarging
LAYOUT_ORDER = ["odd-offset", "dense", "bottom-up", "padded", "word-offset"]
_MEMBER_REF = {}


def member_case(src_hw, dst_hw, filt):
    key = (src_hw, dst_hw, filt)
    if key not in _MEMBER_REF:
        src = np.random.default_rng(src_hw[0] * 131 + src_hw[1] + 7 * filt).integers(0, 256, src_hw + (4,), dtype=np.uint8)
        _MEMBER_REF[key] = (src, F.scale8(src, dst_hw[0], dst_hw[1], filt))
    return _MEMBER_REF[key]


def scale_members(filts, dsts, dst_hw, srcs, src_hws):
    lib = R.load_library(True)
    n = len(dsts)
    return lib.ju_debug_scale_members(n, (C.c_int * n)(*filts), (C.c_void_p * n)(*[d.ptr for d in dsts]),
                                      (C.c_ssize_t * n)(*[d.stride for d in dsts]), dst_hw[1], dst_hw[0],
                                      (C.c_void_p * n)(*[s.ptr for s in srcs]), (C.c_ssize_t * n)(*[s.stride for s in srcs]),
                                      (C.c_size_t * n)(*[hw[1] for hw in src_hws]), (C.c_size_t * n)(*[hw[0] for hw in src_hws]))


def check_members(dst_hw, picks):
    """One launch over the (source size, filter) pairs of `picks`; aligned and unaligned layouts mixed over the members."""
    lib = R.load_library(True)
    srcs, dsts = [], []
    for i, (hw, filt) in enumerate(picks):
        srcs.append(DevPlane(member_case(hw, dst_hw, filt)[0], **LAYOUTS[LAYOUT_ORDER[i % 5]]))
        dsts.append(DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **LAYOUTS[LAYOUT_ORDER[(i + 1) % 5]]))
    assert scale_members([f for _, f in picks], dsts, dst_hw, srcs, [hw for hw, _ in picks]) == 0, lib.ju_last_error()
    for i, (hw, filt) in enumerate(picks):
        src, want = member_case(hw, dst_hw, filt)
        dsts[i].check(want)                                      # (and the guard bytes around every row)
        srcs[i].check(src)                                       # the sources: unchanged
    if len(picks) == 1:                                          # the single-frame kernel: the same bytes
        (hw, filt), = picks
        one = DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **LAYOUTS[LAYOUT_ORDER[1]])
        assert lib.ju_debug_scale(0, filt, one.ptr, one.stride, dst_hw[1], dst_hw[0], srcs[0].ptr, srcs[0].stride, hw[1], hw[0],
                                  None, None, None) == 0, lib.ju_last_error()
        assert np.array_equal(one.buf.cpu().numpy(), dsts[0].buf.cpu().numpy())


@pytest.mark.parametrize("count", [1, 2, 3, 8])
def test_members_of_different_sizes_and_filters_share_one_launch(count):
    for shift in range(3 if count == 1 else 2):                  # (count 1: each filter's form alone)
        check_members((16, 24), [(MEMBER_SIZES[(i + shift) % 5], F.FILTERS[(i + shift) % 3]) for i in range(count)])


def test_the_widest_tile_beside_the_narrowest():
    """(64, 1920) -> (16, 480) needs the largest LDS tile of the launch, (16, 480) passing through the smallest: a member
    addresses its rows by its own pitch, whatever the launch's LDS size."""
    wide, narrow = (64, 1920), (16, 480)
    for order in ([wide, narrow], [narrow, wide]):
        for filts in ((F.TRIANGLE, F.MITCHELL), (F.CATMULL_ROM, F.TRIANGLE)):
            check_members((16, 480), list(zip(order, filts)))


def test_the_members_hook_refuses_bad_arguments():
    lib = R.load_library(True)
    fake = (C.c_void_p * 9)(*([0x1000] * 9))                     # (never read: every case is refused before a device call)
    null, strides, filts = (C.c_void_p * 9)(), (C.c_ssize_t * 9)(), (C.c_int * 9)()
    widths, heights = (C.c_size_t * 9)(*([46] * 9)), (C.c_size_t * 9)(*([30] * 9))

    def call(count, dst=fake, src=fake, filters=filts, w=widths):
        rc = lib.ju_debug_scale_members(count, filters, dst, strides, 24, 16, src, strides, w, heights)
        return rc, lib.ju_last_error().decode() if rc else ""

    for count in (0, -1, 9):
        assert call(count) == (1, "std::invalid_argument: ju_debug_scale_members: count must be 1 .. 8")
    assert call(2, dst=None) == (1, "std::invalid_argument: ju_debug_scale_members: NULL array")
    assert call(2, filters=None) == (1, "std::invalid_argument: ju_debug_scale_members: NULL array")
    assert call(2, src=null) == (1, "std::invalid_argument: ju_debug_scale_members: NULL buffer")
    # a cubic member beyond a factor of 8 beside a triangle member inside its 16
    cubic = (C.c_int * 9)(F.TRIANGLE, F.CATMULL_ROM)
    rc, msg = call(2, filters=cubic, w=(C.c_size_t * 9)(24 * 9, 24 * 9))
    assert rc == 1 and "216 -> 24 is beyond a factor of 8" in msg, msg


# ---- 2. the sized decode launch alone -------------------------------------------------------------------------------------
def decode_items(hook_sized, fmts, css, sizes, outs, srcs):
    lib = R.load_library(True)
    n = len(fmts)
    ptrs, strides = [], []
    for planes in srcs:
        ptrs += [p.ptr for p in planes] + [None] * (3 - len(planes))
        strides += [p.stride for p in planes] + [0] * (3 - len(planes))
    common = ((C.c_void_p * n)(*[o.ptr for o in outs]), (C.c_ssize_t * n)(*[o.stride for o in outs]),
              (C.c_void_p * (3 * n))(*ptrs), (C.c_ssize_t * (3 * n))(*strides))
    if hook_sized:
        rc = lib.ju_debug_yuv_items_sized(n, (C.c_int * n)(*fmts), (C.c_int * n)(*css), (C.c_size_t * n)(*[hw[1] for hw in sizes]),
                                          (C.c_size_t * n)(*[hw[0] for hw in sizes]), *common)
    else:
        (h, w), = set(sizes)
        rc = lib.ju_debug_yuv_items(n, (C.c_int * n)(*fmts), (C.c_int * n)(*css), w, h, *common)
    assert rc == 0, lib.ju_last_error()


# (h, w): the model's input and the two source sizes of the passes below; V210 at a width of whole groups (48) and one with
# a partial group (50); the largest item first, last and in the middle
SIZED_LAUNCHES = [[(NV12, (30, 48)), (P010, (48, 72)), (YUY2, (34, 50))],
                  [(V210, (30, 48)), (V210, (34, 50)), (NV12, (48, 72))],
                  [(P010, (48, 72)), (YUY2, (30, 48)), (NV12, (34, 50)), (V210, (30, 48))],
                  [(YUY2, (34, 50))]]


@pytest.mark.parametrize("launch", range(len(SIZED_LAUNCHES)))
def test_the_sized_decode_launch_equals_the_launch_of_one_size_per_item(launch):
    rng = np.random.default_rng(77 + launch)
    items = SIZED_LAUNCHES[launch]
    fmts, sizes = [f for f, _ in items], [hw for _, hw in items]
    css = [(i + launch) % 4 for i in range(len(items))]
    lays = [PK.RG.layout(PK.RG.LAYOUT_NAMES[(i + launch) % 5], PK.blank(f, 2, 12)[0].dtype.itemsize) for i, f in enumerate(fmts)]
    held = [[rng.integers(0, 256, (p.shape[0], p[0].nbytes), dtype=np.uint8) for p in PK.blank(f, h, w)] for f, (h, w) in items]
    srcs = [[DevPlane(p, **lay) for p in planes] for planes, lay in zip(held, lays)]

    def images():
        return [DevPlane(np.full((h, w, 4), 0x5A, np.uint8), pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
                for (h, w), lay in zip(sizes, lays)]

    outs, singles = images(), images()
    decode_items(True, fmts, css, sizes, outs, srcs)
    for i in range(len(items)):
        decode_items(False, [fmts[i]], [css[i]], [sizes[i]], [singles[i]], [srcs[i]])
        want = singles[i]._rows(singles[i].buf.cpu().numpy()).reshape(sizes[i] + (4,))
        assert want.any() and want[..., 3].max() == 0, i
        singles[i].check(want)
        outs[i].check(want)                                      # the same bytes, the guard bytes untouched
        for p, d in zip(srcs[i], held[i]):
            p.check(d)


# ---- 3. group passes equal the members sent one by one -------------------------------------------------------------------
@dataclasses.dataclass
class Member:
    setup: Setup
    spec: Spec
    ride: int = 1                        # ju_set_stage_group
    scene: int = R.SCENE_OFF             # with ju_set_scene_group(1) when not off

    def configure(self, rt, group=True):
        self.setup.apply(rt)
        if self.scene != R.SCENE_OFF:
            rt.set_scene_detect(self.scene, 10000)
            if group:
                rt.set_scene_group(1)
        if group and self.ride:
            rt.set_stage_group(1)

    @property
    def staged(self):
        return bool(self.setup.src or self.setup.mask or self.setup.out)


MEMBERS = [
    Member(Setup(), Spec(BGRX, "device", "plain", BGRX, "device", "plain")),                       # a plain lead
    Member(Setup(src=SRC), Spec(BGRX, "device", "odd", BGRX, "device", "padded")),                 # off every alignment
    Member(Setup(src=SRC_ODD, src_filter=F.CATMULL_ROM, out=(90, 130)), Spec(NV12, "host", "padded", P010, "host", "plain")),
    Member(Setup(mask=True), Spec(BGRX, "device", "padded", BGRX, "device", "bottom-up")),
    Member(Setup(src=SRC, src_filter=F.MITCHELL, mask=True, out=(180, 288), out_filter=F.MITCHELL),
           Spec(Y210, "device", "plain", Y210, "device", "padded")),
    Member(Setup(out=(80, 128)), Spec(BGRX, "host", "bottom-up", BGRX, "host", "bottom-up")),
]
# what a frame went through, whichever route it took
ROUTE_FREE_STATS = ("source_stage_frames", "scene_frames", "scene_cuts", "scene_detector_runs", "fallbacks", "lookahead_frames")


def clip_of(member, cfg, ticks, seed):
    (ih, iw), _ = member.setup.sizes(cfg)
    return M.synthetic_frames(ticks, ih, iw, seed=seed, kind="smooth")


def twin_of(blob, dtype, member, clip):
    """ju_process_frame per frame on plain host planes: the outputs, the state and history, the records, the stats."""
    cfg, _ = M.deserialize(blob)
    _, (oh, ow) = member.setup.sizes(cfg)
    want = []
    with R.Runtime(blob, 0, dtype) as rt:
        member.configure(rt, group=False)
        for f in clip:
            pin, pout = PK.source(f, member.spec.fin, CS), PK.blank(member.spec.fout, oh, ow)
            rt.process_frame(R.host_frame(member.spec.fin, pin, CS), R.host_frame(member.spec.fout, pout, CS))
            want.append(pout)
        return want, snapshot(rt), rt.scene_info(), [rt.stat(k) for k in ROUTE_FREE_STATS]


def sides_of(members, cfg, frames):
    ins, outs = [], []
    for mb, f in zip(members, frames):
        (ih, iw), (oh, ow) = mb.setup.sizes(cfg)
        s = mb.spec
        ins.append(Side(s.fin, s.lin, s.layin, PK.source(f, s.fin, CS), iw, ih))
        outs.append(Side(s.fout, s.lout, s.layout, PK.blank(s.fout, oh, ow), ow, oh))
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def check_group(members, ticks, dtype=DTYPE, cfg=None, wts=None, clips=None, in_pass=None, before=None, rerun=False):
    """The members driven through ju_process_group_frames against their twins.  in_pass: which members' frames a pass takes
    (default all)."""
    cfg = cfg or small_config()
    blob = blob_of(cfg, wts)
    clips = clips or [clip_of(mb, cfg, ticks, 31 + k) for k, mb in enumerate(members)]
    twins = [twin_of(blob, dtype, mb, clip) for mb, clip in zip(members, clips)]
    in_pass = [True] * len(members) if in_pass is None else in_pass
    rts = [R.Runtime(blob, 0, dtype) for _ in members]
    try:
        for mb, rt in zip(members, rts):
            assert rt.stat("stage_group") == 0
            mb.configure(rt)
            assert rt.stat("stage_group") == mb.ride and rt.stat("group_staged_frames") == 0
        if before:
            before(rts)
        for t in range(ticks):
            ins, outs = sides_of(members, cfg, [clip[t] for clip in clips])
            R.process_group_frames(rts, [x.frame for x in ins], [x.frame for x in outs])
            for k in range(len(members)):
                outs[k].check(twins[k][0][t])                    # every plane, and the guard bytes around it
                ins[k].untouched()
        for k, (mb, rt) in enumerate(zip(members, rts)):
            assert same_as(rt, twins[k][1]), k
            assert rt.scene_info() == twins[k][2], k
            assert [rt.stat(s) for s in ROUTE_FREE_STATS] == twins[k][3], k
            rode = ticks if in_pass[k] and not rerun else 0
            assert rt.stat("group_frames") == rode, k
            assert rt.stat("group_staged_frames") == (rode if mb.staged and mb.ride else 0), k
            assert rt.stat("group_yuv_frames") == (rode if (mb.spec.fin, mb.spec.fout) != (BGRX, BGRX) else 0), k
            if mb.scene != R.SCENE_OFF:
                assert rt.stat("scene_group_frames") == rode, k
        return twins
    finally:
        for rt in rts:
            rt.close()


def test_six_members_with_their_own_stages_equal_their_twins():
    check_group(MEMBERS, 5)


# ---- 4. variants ------------------------------------------------------------------------------------------------------------
def test_a_staged_member_as_lead():
    check_group([MEMBERS[4], MEMBERS[0], MEMBERS[3], MEMBERS[2]], 3)


def test_a_staged_member_that_detects_restarts_at_its_cut_inside_the_pass():
    cfg = small_config()
    members = [MEMBERS[0], dataclasses.replace(MEMBERS[4], scene=R.SCENE_RESET), dataclasses.replace(MEMBERS[1], scene=R.SCENE_REPORT)]
    clips = [clip_of(mb, cfg, 3, 31 + k) for k, mb in enumerate(members)]
    for k in (1, 2):                                             # a cut at tick 2, at source size
        other = M.synthetic_frames(3, SRC[0], SRC[1], seed=77 + k, kind="smooth")
        clips[k] = [clips[k][0], clips[k][1], 255 - other[2]]
    twins = check_group(members, 3, clips=clips)
    assert [r["cut"] for r in twins[1][2]] == [0, 0, 1] and [r["cut"] for r in twins[2][2]] == [0, 0, 1]
    # the restart is visible: the resetting twin's state differs from the state of the same member without a detector
    plain = twin_of(blob_of(cfg), DTYPE, MEMBERS[4], clips[1])
    assert not np.array_equal(plain[1][0], twins[1][1][0])


def test_a_flow_free_model():
    cfg, wts = flow_free(small_config())
    check_group([MEMBERS[0], MEMBERS[2], MEMBERS[4], MEMBERS[5]], 3, cfg=cfg, wts=wts)


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_both_dtypes(dtype):
    check_group([MEMBERS[1], MEMBERS[4], MEMBERS[2]], 3, dtype=dtype)


def test_a_pass_that_is_run_again_gives_the_same_bytes():
    lib = R.load_library(True)
    assert lib.ju_debug_set(b"group_rerun", 1) == 0
    try:
        check_group([MEMBERS[0], MEMBERS[4], MEMBERS[2], MEMBERS[3]], 3, rerun=True)
    finally:
        lib.ju_debug_set(b"group_rerun", 0)


def test_a_call_longer_than_the_leads_cap_splits_into_passes():
    """5 members under a cap of 2: passes of 2 and 2, and the fifth on its own."""
    members = [MEMBERS[1], MEMBERS[0], MEMBERS[4], MEMBERS[2], MEMBERS[5]]
    check_group(members, 3, before=lambda rts: rts[0].set_lookahead(2), in_pass=[True, True, True, True, False])


# ---- 5. settings changed between calls --------------------------------------------------------------------------------------
def test_settings_changed_and_a_member_destroyed_between_calls_leave_no_stale_slot():
    cfg = small_config()
    blob = blob_of(cfg)
    steps = [Setup(src=SRC, out=(90, 130)), Setup(src=SRC_ODD, mask=True, out=(90, 130)), Setup(src=SRC_ODD, mask=True, out=(180, 288)),
             Setup(mask=True, out=(80, 128)), Setup(src=SRC, src_filter=F.MITCHELL), Setup(src=SRC, src_filter=F.MITCHELL)]
    spec = Spec(NV12, "host", "plain", P010, "device", "padded")       # every slot kind of a member: planes, 8 and 16 bit
    other = MEMBERS[4]

    def configure(rt, s):
        rt.set_source_size(*((s.src[1], s.src[0], s.src_filter) if s.src else (0, 0, 0)))
        rt.set_source_mask(make_mask((37, 50), 2) if s.mask else None)
        rt.set_output_size(*((s.out[1], s.out[0], s.out_filter) if s.out else (0, 0, 0)))

    names = ("lead", "changing", "other")
    rts = {k: R.Runtime(blob, 0, DTYPE) for k in names}
    twins = {k: R.Runtime(blob, 0, DTYPE) for k in names}
    try:
        other.setup.apply(rts["other"])
        other.setup.apply(twins["other"])
        rts["other"].set_stage_group(1)
        rts["changing"].set_stage_group(1)
        staged = 0
        for t, s in enumerate(steps):
            if t == 2:                                           # a member that owned slots goes away between ticks
                rts.pop("other").close()
                twins.pop("other").close()
            if t == 5:                                           # the setting off again: alone, the counters stand still
                rts["changing"].set_stage_group(0)
            configure(rts["changing"], s)
            configure(twins["changing"], s)
            live = [k for k in names if k in rts]
            members = [{"lead": MEMBERS[0], "changing": Member(s, spec), "other": other}[k] for k in live]
            frames = [clip_of(mb, cfg, 1, 100 + 7 * t + i)[0] for i, mb in enumerate(members)]
            ins, outs = sides_of(members, cfg, frames)
            R.process_group_frames([rts[k] for k in live], [x.frame for x in ins], [x.frame for x in outs])
            for i, (k, mb) in enumerate(zip(live, members)):
                _, (oh, ow) = mb.setup.sizes(cfg)
                pin, pout = PK.source(frames[i], mb.spec.fin, CS), PK.blank(mb.spec.fout, oh, ow)
                twins[k].process_frame(R.host_frame(mb.spec.fin, pin, CS), R.host_frame(mb.spec.fout, pout, CS))
                outs[i].check(pout)
                ins[i].untouched()
                assert same_as(rts[k], snapshot(twins[k])), (t, k)
            staged += 1 if t < 5 else 0
            assert rts["changing"].stat("group_staged_frames") == rts["changing"].stat("group_frames") == staged, t
            assert rts["changing"].stat("source_stage_frames") == t + 1
            assert rts["lead"].stat("group_frames") == (t + 1 if t < 5 else 5)   # (tick 5: no second member for a pass)
    finally:
        for rt in list(rts.values()) + list(twins.values()):
            rt.close()


# ---- 6. refusals and routing ------------------------------------------------------------------------------------------------
STAT_KEYS = ("group_frames", "group_yuv_frames", "group_staged_frames", "source_stage_frames", "graph_replays", "eager_runs",
             "lookahead_frames", "fallbacks")


def test_refusals_and_routing():
    cfg = small_config()
    blob = blob_of(cfg)
    lib = R.load_library(True)
    members = [MEMBERS[0], MEMBERS[1], dataclasses.replace(MEMBERS[4], ride=0), MEMBERS[3]]
    rts = [R.Runtime(blob, 0, DTYPE) for _ in members]
    try:
        for mb, rt in zip(members, rts):
            mb.configure(rt)
        # bad values of `on`: the exact message, the setting as it was
        for bad in (2, -1, 7):
            with pytest.raises(R.JoshUpscaleError) as e:
                rts[1].set_stage_group(bad)
            assert e.value.code == 1
            assert e.value.message == f"std::invalid_argument: ju_set_stage_group: on must be 0 or 1, got {bad}"
            assert lib.ju_set_stage_group(rts[1]._h, bad) == 1
        assert rts[1].stat("stage_group") == 1
        rts[1].reset()
        assert rts[1].stat("stage_group") == 1                   # (ju_reset keeps the setting)
        # one tick: the member with the setting 0 runs alone beside the pass of the other three
        clips = [clip_of(mb, cfg, 2, 51 + k) for k, mb in enumerate(members)]
        twins = [twin_of(blob, DTYPE, mb, clip[:1]) for mb, clip in zip(members, clips)]
        ins, outs = sides_of(members, cfg, [clip[0] for clip in clips])
        R.process_group_frames(rts, [x.frame for x in ins], [x.frame for x in outs])
        for k in range(4):
            outs[k].check(twins[k][0][0])
            assert same_as(rts[k], twins[k][1]), k
        assert [rt.stat("group_frames") for rt in rts] == [1, 1, 0, 1]
        assert [rt.stat("group_staged_frames") for rt in rts] == [0, 1, 0, 1]
        assert [rt.stat("source_stage_frames") for rt in rts] == [0, 1, 1, 1]
        # a riding member's frame at the model's size while its source size is set: refused, the member named, nothing moved
        before = [(snapshot(rt), [rt.stat(k) for k in STAT_KEYS]) for rt in rts]
        ins2, outs2 = sides_of(members, cfg, [clip[1] for clip in clips])
        small = Side(BGRX, "device", "plain", [np.zeros((cfg.frame_height, cfg.frame_width, 4), np.uint8)], cfg.frame_width,
                     cfg.frame_height)
        with pytest.raises(R.JoshUpscaleError) as e:
            R.process_group_frames(rts, [ins2[0].frame, small.frame, ins2[2].frame, ins2[3].frame], [x.frame for x in outs2])
        assert e.value.code == 1 and "member 1" in e.value.message and "exactly 72x48 (the source size set)" in e.value.message
        for rt, (snap, stats) in zip(rts, before):
            assert same_as(rt, snap) and [rt.stat(k) for k in STAT_KEYS] == stats
        for x in outs2:
            x.untouched()
    finally:
        for rt in rts:
            rt.close()


def test_an_output_at_output_size_over_another_members_source_sends_the_call_member_by_member():
    """Member 0's output at its output size, 288 x 180, reaches beyond the model-size 192 x 120 frame; member 1's 72 x 48
    source lies in that reach.  In list order member 0 writes before member 1 reads: only member by member gives those bytes."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    out_hw, at = (180, 288), 150000
    assert 4 * h * 4 * w * 4 < at and at + SRC[0] * SRC[1] * 4 <= out_hw[0] * out_hw[1] * 4
    frames = [M.synthetic_frames(1, h, w, seed=3, kind="smooth")[0], M.synthetic_frames(1, SRC[0], SRC[1], seed=4, kind="smooth")[0]]

    def run(group):
        shared = torch.zeros(out_hw[0] * out_hw[1] * 4, dtype=torch.uint8, device=dev)
        shared[at:at + frames[1].size] = torch.from_numpy(frames[1].reshape(-1)).to(dev)
        in0 = torch.from_numpy(frames[0]).to(dev)
        out1 = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rts = [R.Runtime(blob, 0, DTYPE) for _ in range(2)]
        try:
            rts[0].set_output_size(out_hw[1], out_hw[0])
            rts[1].set_source_size(SRC[1], SRC[0])
            ins = [R.device_frame(BGRX, w, h, [in0]), R.device_frame(BGRX, SRC[1], SRC[0], [shared.data_ptr() + at])]
            outs = [R.device_frame(BGRX, out_hw[1], out_hw[0], [shared]), R.device_frame(BGRX, 4 * w, 4 * h, [out1])]
            if group:
                for rt in rts:
                    rt.set_stage_group(1)
                R.process_group_frames(rts, ins, outs)
                assert [rt.stat("group_frames") for rt in rts] == [0, 0]
                assert [rt.stat("source_stage_frames") for rt in rts] == [1, 1]
            else:
                for rt, i, o in zip(rts, ins, outs):
                    rt.process_frame(i, o)
            return shared.cpu().numpy(), out1.cpu().numpy(), [snapshot(rt) for rt in rts]
        finally:
            for rt in rts:
                rt.close()

    got, want = run(True), run(False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].any()
    for a, b in zip(got[2], want[2]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
