"""Scaled and masked frames inside look-ahead passes (ju_set_stage_lookahead; docs/source_stage.md and docs/output_stage.md,
"Passes"): the items kernel alone against the numpy definition and the single-frame kernel, byte for byte; passes against
a twin runtime with the same settings fed frame by frame -- every output byte with its guards, the state and the frame
history -- whose route tests/test_gpu_source.py and tests/test_gpu_output.py hold to the numpy definitions; other model
variants; the scene detector inside staged passes; switching the settings between passes; the refusals."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import scale_filter_reference as F
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_packed10 import Y210, blank, source
from test_gpu_source import LAYOUTS, make_mask
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import as_bytes
from test_gpu_yuv_lookahead import HostPlane

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
BGRX, NV12, P010 = R.FMT_BGRX, R.FMT_NV12, R.FMT_P010
SRC = (48, 72)                           # (h, w) for the 30 x 48 model: 1.6 and 1.5 to one
SRC_ODD = (34, 50)                       # odd ratios, even sizes for the YUV frames
OUT_SIZES = [(80, 128), (180, 288), (90, 130)]
FILTER_IDS = [F.NAMES[f] for f in F.FILTERS]


# ---- 1. the items kernel alone ------------------------------------------------------------------------------------------
ITEM_CASES = [((30, 46), (16, 24)), ((17, 23), (16, 24)), ((8, 12), (16, 24)), ((16, 24), (16, 24)), ((64, 1920), (16, 480)),
              ((64, 1024), (4, 64)), ((4, 6), (64, 96))]
LAYOUT_ORDER = ["odd-offset", "dense", "bottom-up", "padded", "word-offset"]
_ITEM_REF = {}


def item_case(src_hw, dst_hw, filt, i):
    key = (src_hw, dst_hw, filt, i)
    if key not in _ITEM_REF:
        src = np.random.default_rng(src_hw[0] * 131 + src_hw[1] + 7 * i).integers(0, 256, src_hw + (4,), dtype=np.uint8)
        _ITEM_REF[key] = (src, F.scale8(src, dst_hw[0], dst_hw[1], filt))
    return _ITEM_REF[key]


def scale_items(filt, dsts, dst_hw, srcs, src_hw):
    lib = R.load_library(True)
    n = len(dsts)
    rc = lib.ju_debug_scale_items(n, filt, (C.c_void_p * n)(*[d.ptr for d in dsts]), (C.c_ssize_t * n)(*[d.stride for d in dsts]),
                                  dst_hw[1], dst_hw[0], (C.c_void_p * n)(*[s.ptr for s in srcs]),
                                  (C.c_ssize_t * n)(*[s.stride for s in srcs]), src_hw[1], src_hw[0])
    assert rc == 0, lib.ju_last_error()


@pytest.mark.parametrize("filt", F.FILTERS, ids=FILTER_IDS)
def test_items_kernel_equals_the_numpy_definition_and_the_single_frame_kernel(filt):
    lib = R.load_library(True)
    for src_hw, dst_hw in ITEM_CASES:
        if src_hw[0] > F.down_max(filt) * dst_hw[0] or src_hw[1] > F.down_max(filt) * dst_hw[1]:
            continue                                             # (a cubic filter reduces by 8 at the most)
        for count in (1, 2, 3, 8):
            srcs, dsts, wants = [], [], []
            for i in range(count):                               # aligned and unaligned items share the launch
                src, want = item_case(src_hw, dst_hw, filt, i % 3)
                srcs.append(DevPlane(src, **LAYOUTS[LAYOUT_ORDER[i % 5]]))
                dsts.append(DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **LAYOUTS[LAYOUT_ORDER[(i + 1) % 5]]))
                wants.append(want)
            scale_items(filt, dsts, dst_hw, srcs, src_hw)
            for i in range(count):
                dsts[i].check(wants[i])                          # (and the guard bytes around every row)
                srcs[i].check(item_case(src_hw, dst_hw, filt, i % 3)[0])
            if count == 1:                                       # the single-frame launch: the same bytes
                one = DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **LAYOUTS[LAYOUT_ORDER[1]])
                assert lib.ju_debug_scale(0, filt, one.ptr, one.stride, dst_hw[1], dst_hw[0], srcs[0].ptr, srcs[0].stride,
                                          src_hw[1], src_hw[0], None, None, None) == 0, lib.ju_last_error()
                assert np.array_equal(one.buf.cpu().numpy(), dsts[0].buf.cpu().numpy())
                if filt == F.TRIANGLE:
                    two = DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **LAYOUTS[LAYOUT_ORDER[1]])
                    assert lib.ju_debug_source(0, two.ptr, two.stride, dst_hw[1], dst_hw[0], srcs[0].ptr, srcs[0].stride,
                                               src_hw[1], src_hw[0], None, 0, 0, 0) == 0, lib.ju_last_error()
                    assert np.array_equal(two.buf.cpu().numpy(), dsts[0].buf.cpu().numpy())


def test_items_hook_refuses_bad_arguments():
    lib = R.load_library(True)
    ptrs, strides = (C.c_void_p * 9)(), (C.c_ssize_t * 9)()

    def call(count, filt=0, dst=ptrs):
        rc = lib.ju_debug_scale_items(count, filt, dst, strides, 24, 16, ptrs, strides, 46, 30)
        return rc, lib.ju_last_error().decode() if rc else ""

    for count in (0, -1, 9):
        assert call(count) == (1, "std::invalid_argument: ju_debug_scale_items: count must be 1 .. 8")
    assert call(2, dst=None) == (1, "std::invalid_argument: ju_debug_scale_items: NULL array")
    assert call(2) == (1, "std::invalid_argument: ju_debug_scale_items: NULL buffer")


# ---- 2. passes equal the frames sent one by one ---------------------------------------------------------------------------
LAYS = {"plain": dict(pad=0, offset=0, flip=False), "padded": dict(pad=24, offset=0, flip=False),
        "bottom-up": dict(pad=8, offset=0, flip=True), "odd": dict(pad=13, offset=1, flip=False)}


class Side:
    """One side of a frame call: its planes in host or device memory with guard bytes around them."""

    def __init__(self, fmt, loc, layout, planes, w, h):
        lay = dict(LAYS[layout])
        if fmt == BGRX and layout != "odd":
            lay["pad"] *= 4                                      # (device BGRX rows stay 8-byte aligned)
        cls = HostPlane if loc == "host" else DevPlane
        self.fmt = fmt
        self.planes = [cls(p if fmt == BGRX else as_bytes(p), **lay) for p in planes]
        self.frame = R._frame(fmt, CS, R.LOC_CPU if loc == "host" else R.LOC_DEVICE, w, h,
                              [p.ptr for p in self.planes], [p.stride for p in self.planes])

    def check(self, want):
        for p, e in zip(self.planes, want):
            p.check(e if self.fmt == BGRX else as_bytes(e))

    def untouched(self):
        for p in self.planes:
            p.check(p._rows(p.host))


@dataclasses.dataclass
class Spec:
    fin: int
    lin: str
    layin: str
    fout: int
    lout: str
    layout: str


def specs_for(scaled_in, scaled_out):
    """Eleven frames: BGRX, NV12, P010 and Y210 in and out, host and device, bottom-up; device BGRX off every alignment on
    the sides a scaler touches (the plain sides keep the alignment of the plain passes)."""
    odd_in, odd_out = ("odd" if scaled_in else "padded"), ("odd" if scaled_out else "padded")
    return [Spec(BGRX, "device", "plain", BGRX, "device", "plain"),
            Spec(BGRX, "device", "bottom-up", NV12, "host", "padded"),
            Spec(NV12, "host", "plain", BGRX, "host", "bottom-up"),
            Spec(P010, "device", "padded", P010, "device", "plain"),
            Spec(Y210, "host", "bottom-up", Y210, "device", "padded"),
            Spec(BGRX, "host", "bottom-up", P010, "host", "bottom-up"),
            Spec(BGRX, "device", odd_in, BGRX, "device", odd_out),
            Spec(NV12, "device", "padded", Y210, "host", "plain"),
            Spec(P010, "host", "padded", BGRX, "device", "bottom-up"),
            Spec(Y210, "device", "plain", NV12, "device", "bottom-up"),
            Spec(BGRX, "host", "plain", BGRX, "host", "plain")]


@dataclasses.dataclass
class Setup:
    src: tuple = None                    # (h, w) of the source size, or None
    src_filter: int = F.TRIANGLE
    mask: bool = False
    out: tuple = None                    # (h, w) of the output size, or None
    out_filter: int = F.TRIANGLE

    def apply(self, rt):
        if self.src:
            rt.set_source_size(self.src[1], self.src[0], self.src_filter)
        if self.mask:
            rt.set_source_mask(make_mask((37, 50), 2))
        if self.out:
            rt.set_output_size(self.out[1], self.out[0], self.out_filter)

    def sizes(self, cfg):
        return (self.src or (cfg.frame_height, cfg.frame_width)), (self.out or (4 * cfg.frame_height, 4 * cfg.frame_width))


def blob_of(cfg, wts=None):
    return M.serialize(cfg, wts if wts is not None else M.make_seeded_weights(cfg))


def snapshot(rt):
    if not rt.recurrent:
        return None
    return rt.read_tensor("state").copy(), rt.read_tensor("flow_in").copy()


def same_as(rt, snap):
    if snap is None:
        return True
    return np.array_equal(rt.read_tensor("state"), snap[0]) and np.array_equal(rt.read_tensor("flow_in"), snap[1])


def twin_run(blob, dtype, setup, specs, frames, prepare=None):
    """What the frame-by-frame staged route writes for plain host frames, + the state and the history after the last."""
    cfg, _ = M.deserialize(blob)
    (ih, iw), (oh, ow) = setup.sizes(cfg)
    want = []
    with R.Runtime(blob, 0, dtype) as rt:
        setup.apply(rt)
        if prepare:
            prepare(rt)
        for f, s in zip(frames, specs):
            pin, pout = source(f, s.fin, CS), blank(s.fout, oh, ow)   # (kept alive: the frame holds raw pointers)
            rt.process_frame(R.host_frame(s.fin, pin, CS), R.host_frame(s.fout, pout, CS))
            want.append(pout)
        assert rt.stat("lookahead_frames") == 0 and rt.stat("source_stage_frames") == len(frames)
        extra = rt.scene_info(len(frames)) if prepare else None
        return want, snapshot(rt), extra


def make_sides(setup, cfg, specs, frames):
    (ih, iw), (oh, ow) = setup.sizes(cfg)
    ins = [Side(s.fin, s.lin, s.layin, source(f, s.fin, CS), iw, ih) for f, s in zip(frames, specs)]
    outs = [Side(s.fout, s.lout, s.layout, blank(s.fout, oh, ow), ow, oh) for s in specs]
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def run_calls(rt, ins, outs, want, lengths):
    t = 0
    for k in lengths:
        rt.process_frames([x.frame for x in ins[t:t + k]], [x.frame for x in outs[t:t + k]])
        for i in range(t, t + k):
            outs[i].check(want[i])                               # (every output byte, guard bytes included)
        t += k
    assert t == len(ins)


def clip_for(setup, cfg, n, seed):
    (ih, iw), _ = setup.sizes(cfg)
    return M.synthetic_frames(n, ih, iw, seed=seed, kind="smooth")


def check_passes(setup, dtype=R.DTYPE_F16, cfg=None, wts=None, n=11, lengths=((11,), (2, 2, 2, 2, 2, 1)), in_passes=(11, 10),
                 expect_passes=True, seed=5):
    cfg = cfg or small_config()
    blob = blob_of(cfg, wts)
    specs = specs_for(setup.src is not None, setup.out is not None)[:n]
    frames = clip_for(setup, cfg, n, seed)
    want, snap, _ = twin_run(blob, dtype, setup, specs, frames)
    ins, outs = make_sides(setup, cfg, specs, frames)
    with R.Runtime(blob, 0, dtype) as a:
        setup.apply(a)
        assert a.stat("stage_lookahead") == 0
        a.set_stage_lookahead(1)
        assert a.stat("stage_lookahead") == 1 and a.stat("lookahead_staged_frames") == 0
        total = 0
        for chunks, counted in zip(lengths, in_passes):
            a.reset()
            assert a.stat("stage_lookahead") == 1                # (ju_reset keeps the setting)
            run_calls(a, ins, outs, want, chunks)
            assert same_as(a, snap), chunks
            if expect_passes and total == 0 and counted == n:    # (the first run, every frame in a pass)
                assert a.stat("lookahead_host_frames") == sum(1 for s in specs if "host" in (s.lin, s.lout))
                assert a.stat("lookahead_yuv_frames") == sum(1 for s in specs if BGRX != s.fin or BGRX != s.fout)
            total += counted if expect_passes else 0
            assert a.stat("lookahead_frames") == a.stat("lookahead_staged_frames") == total, chunks
        assert a.stat("fallbacks") == 0
        for x in ins:
            x.untouched()                                        # (the sources and their guards: read only)
        if expect_passes:
            # the same buffers again: captured at the second use, replayed from then on without a capture
            chunks = lengths[0]
            for run in range(2):
                captures, replays = a.stat("graph_captures"), a.stat("graph_replays")
                a.reset()
                run_calls(a, ins, outs, want, chunks)
                assert same_as(a, snap)
            assert a.stat("graph_captures") == captures and a.stat("graph_replays") > replays
        assert a.stat("source_stage_frames") == n * (len(lengths) + (2 if expect_passes else 0))


@pytest.mark.parametrize("filt", F.FILTERS, ids=FILTER_IDS)
def test_a_source_size_alone(filt):
    check_passes(Setup(src=SRC, src_filter=filt))


def test_an_odd_source_size_in_bf16():
    check_passes(Setup(src=SRC_ODD), dtype=R.DTYPE_BF16, lengths=((11,),), in_passes=(11,))


def test_a_mask_alone():
    """(the frames 0, 6 and 8: device BGRX outputs blended in place)"""
    check_passes(Setup(mask=True))


@pytest.mark.parametrize("out,filt", list(zip(OUT_SIZES, F.FILTERS)) + [(OUT_SIZES[1], F.TRIANGLE)],
                         ids=["80x128-triangle", "180x288-catmull-rom", "90x130-mitchell", "180x288-triangle"])
def test_an_output_size_alone(out, filt):
    """(the P010 and Y210 outputs: from this frame's link of the state chain, scaled in 16 bits)"""
    check_passes(Setup(out=out, out_filter=filt), lengths=((11,),), in_passes=(11,))


def test_all_three_settings_together():
    """(deep outputs under a mask: from the blended, scaled 8-bit frame)"""
    check_passes(Setup(src=SRC, mask=True, out=OUT_SIZES[2], src_filter=F.CATMULL_ROM, out_filter=F.MITCHELL))


def test_all_three_settings_at_an_odd_source_size():
    check_passes(Setup(src=SRC_ODD, mask=True, out=OUT_SIZES[0]), lengths=((11,),), in_passes=(11,))


def test_process_batch_takes_staged_device_and_host_images():
    cfg = small_config()
    blob = blob_of(cfg)
    setup = Setup(src=SRC, mask=True, out=OUT_SIZES[1])
    (ih, iw), (oh, ow) = setup.sizes(cfg)
    specs = [Spec(BGRX, "device", "odd", BGRX, "device", "odd"), Spec(BGRX, "host", "bottom-up", BGRX, "host", "padded"),
             Spec(BGRX, "device", "bottom-up", BGRX, "host", "bottom-up"), Spec(BGRX, "host", "plain", BGRX, "device", "plain"),
             Spec(BGRX, "device", "plain", BGRX, "device", "bottom-up")]
    frames = clip_for(setup, cfg, 5, 23)
    want, snap, _ = twin_run(blob, R.DTYPE_F16, setup, specs, frames)
    ins, outs = make_sides(setup, cfg, specs, frames)

    def image(side, w, h):
        p = side.planes[0]
        return R.JuImage(p.ptr, R.LOC_CPU if isinstance(p, HostPlane) else R.LOC_DEVICE, p.stride, w, h)

    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        setup.apply(a)
        a.set_stage_lookahead(1)
        a.process_batch([image(x, iw, ih) for x in ins], [image(x, ow, oh) for x in outs])
        for i in range(5):
            outs[i].check(want[i])
        assert same_as(a, snap)
        assert a.stat("lookahead_frames") == a.stat("lookahead_staged_frames") == 5 and a.stat("lookahead_host_frames") == 3


# ---- 3. model variants, in passes of 3 with all three settings -----------------------------------------------------------
def variant(name):
    if name == "flow-free":
        return flow_free(small_config())
    cfg = {"brightness": small_config(normalize_brightness=True), "output-flow": small_config(output="pre_warp"),
           "temporal": small_config(temporal_strength=0.25)}[name]
    return cfg, None


@pytest.mark.parametrize("name", ["flow-free", "brightness", "output-flow", "temporal"])
def test_model_variants_in_passes_of_three(name):
    cfg, wts = variant(name)
    # (a normalize_brightness model forms no passes at all: its frames take the staged route and the bytes must still agree)
    check_passes(Setup(src=SRC, mask=True, out=OUT_SIZES[0]), cfg=cfg, wts=wts, n=6, lengths=((3, 3),),
                 in_passes=(6,), expect_passes=name != "brightness", seed=31)


def test_a_pre_warp_models_deep_outputs_without_a_mask():
    """hbd_from_state 0: P010 and Y210 under an output size come from the scaled 8-bit frame."""
    check_passes(Setup(out=OUT_SIZES[1]), cfg=small_config(output="pre_warp"), n=6, lengths=((3, 3),), in_passes=(6,), seed=37)


# ---- 4. with the scene detector ----------------------------------------------------------------------------------------
def test_the_scene_detector_reads_the_scaled_frame_inside_staged_passes():
    cfg = small_config()
    blob = blob_of(cfg)
    setup = Setup(src=SRC, mask=True, out=OUT_SIZES[0])
    a_part, b_part = M.synthetic_frames(11, SRC[0], SRC[1], seed=3, kind="smooth"), M.synthetic_frames(11, SRC[0], SRC[1], seed=77, kind="smooth")
    frames = [a_part[t] if t < 3 or 6 <= t < 9 else 255 - b_part[t] for t in range(11)]   # cuts at 3, 6 and 9
    specs = specs_for(True, True)
    detect = lambda rt: rt.set_scene_detect(R.SCENE_RESET, 10000)  # noqa: E731
    want, snap, records = twin_run(blob, R.DTYPE_F16, setup, specs, frames, prepare=detect)
    cuts = [r["step"] for r in records if r["cut"]]              # (the twin's decisions are the reference; the content cuts
    assert {3, 6, 9} <= set(cuts) and 0 not in cuts and 4 not in cuts   # inside both passes, 8 + 3, and not everywhere)
    ins, outs = make_sides(setup, cfg, specs, frames)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        setup.apply(a)
        detect(a)
        a.set_scene_lookahead(1)
        a.set_stage_lookahead(1)
        for run in range(3):                                     # eager, captured, replayed
            if run:
                a.reset()
                a.set_scene_detect(R.SCENE_OFF, 0)               # (the detector's steps start at 0 again, as the twin's)
                detect(a)
            run_calls(a, ins, outs, want, (11,))
            assert same_as(a, snap), run
            assert a.scene_info(11) == records, run
        assert a.stat("scene_pass_frames") == a.stat("lookahead_staged_frames") == a.stat("lookahead_frames") == 33
        assert a.stat("fallbacks") == 0


# ---- 5. switching ------------------------------------------------------------------------------------------------------
def test_switching_the_settings_between_passes_replays_no_stale_graph():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    n = 4
    big = {hw: torch.from_numpy(np.stack(M.synthetic_frames(n, hw[0], hw[1], seed=41, kind="smooth"))).to(dev)
           for hw in (SRC, (h, w))}
    d_out = torch.zeros((n, 4 * h * 4 * w * 4), dtype=torch.uint8, device=dev)   # (one allocation serves every output size)
    torch.cuda.synchronize()
    steps = [Setup(src=SRC), Setup(src=SRC, src_filter=F.MITCHELL), Setup(src=SRC, mask=True), Setup(src=SRC, mask=True, out=(90, 130)),
             Setup(src=SRC, mask=True, out=(80, 128)), Setup(mask=True, out=(80, 128)), Setup(out=(80, 128)), Setup(src=SRC)]

    def configure(rt, s):
        rt.set_source_size(*((s.src[1], s.src[0], s.src_filter) if s.src else (0, 0, 0)))
        rt.set_source_mask(make_mask((37, 50), 2) if s.mask else None)
        rt.set_output_size(*((s.out[1], s.out[0], s.out_filter) if s.out else (0, 0, 0)))

    def images(rt, s):
        (ih, iw), (oh, ow) = s.sizes(cfg)
        return ([rt.device_image(big[(ih, iw)][k].data_ptr(), iw, ih) for k in range(n)],
                [rt.device_image(d_out[k].data_ptr(), ow, oh) for k in range(n)]), oh * ow * 4

    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        a.set_stage_lookahead(1)
        staged = 0
        for s in steps:
            configure(a, s)
            with R.Runtime(blob, 0, R.DTYPE_F16) as b:           # a fresh twin, frame by frame
                configure(b, s)
                (ins, outs), size = images(b, s)
                d_out.zero_()
                for k in range(n):
                    b.process(ins[k], outs[k])
                want, snap = d_out.cpu().numpy()[:, :size].copy(), snapshot(b)
            for rep in range(3):                                 # eager, captured, replayed: then the setting changes
                a.reset()
                d_out.zero_()
                (ins, outs), size = images(a, s)
                a.process_batch(ins, outs)
                assert np.array_equal(d_out.cpu().numpy()[:, :size], want), (s, rep)
                assert same_as(a, snap), (s, rep)
                staged += n
                assert a.stat("lookahead_staged_frames") == a.stat("lookahead_frames") == staged
        # the setting off: the frames run one by one again, and the counters stand still
        a.set_stage_lookahead(0)
        assert a.stat("stage_lookahead") == 0
        a.reset()
        a.process_batch(ins, outs)
        assert np.array_equal(d_out.cpu().numpy()[:, :size], want) and same_as(a, snap)
        assert a.stat("lookahead_staged_frames") == a.stat("lookahead_frames") == staged
        # on again, and every stage setting off: plain passes, which count as passes but not as staged ones
        a.set_stage_lookahead(1)
        configure(a, Setup())
        with R.Runtime(blob, 0, R.DTYPE_F16) as b:
            (ins, outs), size = images(b, Setup())
            for k in range(n):
                b.process(ins[k], outs[k])
            want, snap = d_out.cpu().numpy()[:, :size].copy(), snapshot(b)
        a.reset()
        d_out.zero_()
        (ins, outs), size = images(a, Setup())
        a.process_batch(ins, outs)
        assert np.array_equal(d_out.cpu().numpy()[:, :size], want) and same_as(a, snap)
        assert a.stat("lookahead_frames") == staged + n and a.stat("lookahead_staged_frames") == staged


def test_refusals_leave_state_and_stats_as_they_were():
    cfg = small_config()
    blob = blob_of(cfg)
    setup = Setup(src=SRC, out=OUT_SIZES[0])
    (ih, iw), (oh, ow) = setup.sizes(cfg)
    frames = clip_for(setup, cfg, 4, 9)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        setup.apply(a)
        a.set_stage_lookahead(1)
        outs = [np.zeros((oh, ow, 4), np.uint8) for _ in range(4)]
        a.process_batch([R.host_image(f) for f in frames[:2]], [R.host_image(o) for o in outs[:2]])
        snap = snapshot(a)
        keys = ("lookahead_frames", "lookahead_staged_frames", "source_stage_frames", "graph_replays", "eager_runs")
        stats = [a.stat(k) for k in keys]
        assert stats[:3] == [2, 2, 2]
        # a wrong-size frame in the middle of a batch: refused before anything is launched
        small = np.zeros((cfg.frame_height, cfg.frame_width, 4), np.uint8)
        for o in outs:
            o[...] = 0x33
        with pytest.raises(R.JoshUpscaleError) as e:
            a.process_batch([R.host_image(frames[0]), R.host_image(frames[1]), R.host_image(small), R.host_image(frames[3])],
                            [R.host_image(o) for o in outs])
        assert e.value.code == 1 and "frame 2" in e.value.message and "exactly 72x48" in e.value.message
        wrong_out = np.zeros((4 * cfg.frame_height, 4 * cfg.frame_width, 4), np.uint8)
        with pytest.raises(R.JoshUpscaleError) as e:
            a.process_batch([R.host_image(f) for f in frames[:3]], [R.host_image(outs[0]), R.host_image(wrong_out), R.host_image(outs[2])])
        assert e.value.code == 1 and "frame 1" in e.value.message and "exactly 128x80" in e.value.message
        assert all((o == 0x33).all() for o in outs) and same_as(a, snap) and [a.stat(k) for k in keys] == stats
        # bad values of `on`: the exact message, the setting as it was
        for bad in (2, -1, 7):
            with pytest.raises(R.JoshUpscaleError) as e:
                a.set_stage_lookahead(bad)
            assert e.value.code == 1
            assert e.value.message == f"std::invalid_argument: ju_set_stage_lookahead: on must be 0 or 1, got {bad}"
            assert lib.ju_set_stage_lookahead(a._h, bad) == 1
        assert a.stat("stage_lookahead") == 1
        # ju_prepare_batch captures nothing while a stage setting is on
        torch, dev = torch_dev()
        d_in = torch.from_numpy(np.stack(frames[:2])).to(dev)
        d_out = torch.zeros((2, oh, ow, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        captured = C.c_int(-1)
        ins = (R.JuImage * 2)(*[a.device_image(d_in[k].data_ptr(), iw, ih) for k in range(2)])
        dsts = (R.JuImage * 2)(*[a.device_image(d_out[k].data_ptr(), ow, oh) for k in range(2)])
        assert lib.ju_prepare_batch(a._h, ins, dsts, 2, C.byref(captured)) == 0 and captured.value == 0


def test_a_staged_pass_that_is_run_again_gives_the_same_bytes_and_counts_as_frames():
    """ju_debug_set "pass_rerun": the pass completes, is treated as one that must run again, and its frames go one by one
    through the staged route from inputs the pass left untouched -- the blend in place and the scaled outputs included."""
    cfg = small_config()
    blob = blob_of(cfg)
    setup = Setup(src=SRC, mask=True, out=OUT_SIZES[0])
    specs = specs_for(True, True)
    frames = clip_for(setup, cfg, 11, 13)
    want, snap, _ = twin_run(blob, R.DTYPE_F16, setup, specs, frames)
    ins, outs = make_sides(setup, cfg, specs, frames)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        setup.apply(a)
        a.set_stage_lookahead(1)
        assert lib.ju_debug_set(b"pass_rerun", 1) == 0
        try:
            run_calls(a, ins, outs, want, (11,))
        finally:
            lib.ju_debug_set(b"pass_rerun", 0)
        assert same_as(a, snap)
        assert a.stat("lookahead_frames") == 0 and a.stat("lookahead_staged_frames") == 0 and a.stat("fallbacks") == 0
        assert a.stat("lookahead_host_frames") == 0 and a.stat("lookahead_yuv_frames") == 0
        assert a.stat("source_stage_frames") == 11
        # ju_time_steps "...@pass" behind a staged pass: a plain pass of its own on the staging buffers -- it launches on nothing
        # the staged pass bound (its stage bits, the callers' rows at their own sizes) -- and ends in ju_reset; the next staged
        # pass is again the frames sent one by one
        assert a.time_steps("flow@pass", 1)[1] > 0
        run_calls(a, ins, outs, want, (11,))
        assert same_as(a, snap)
        assert a.stat("lookahead_frames") == 11 and a.stat("lookahead_staged_frames") == 11 and a.stat("fallbacks") == 0
        assert a.stat("source_stage_frames") == 22
        for x in ins:
            x.untouched()
