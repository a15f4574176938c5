"""Alpha inside look-ahead passes and group passes (ju_set_alpha_lookahead, ju_set_alpha_group; docs/alpha.md "Passes").
Byte for byte, no tolerance: every output byte of a pass, guard bytes included, equals the single-frame route's on a
runtime with the same settings and alpha_lookahead 0; that route's slot equals the numpy definition
(tests/alpha_reference.py) and its colour and state equal a twin's in mode 0.  Together with the stages and the scene
detector, across setting changes over the same buffers, in captured and replayed graphs, in a pass made to run again,
and in group passes whose members each bring their own mode, filter and sizes."""

import numpy as np
import pytest

import alpha_reference as A
import scale_filter_reference as F
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_alpha import BGRX, BGRX64, NV12, RGBX, X2RGB10, blank, split, with_alpha
from test_gpu_source import make_mask
from test_gpu_stage_passes import Side, Spec, blob_of, run_calls, same_as, snapshot
from test_gpu_yuv import torch_dev

pytestmark = pytest.mark.gpu

BGR24 = R.FMT_BGR24

# sides rotate over the five formats (NV12 in: opaque; NV12 out: nothing launched) and over host, bottom-up host and device
SPECS = [Spec(BGRX, "device", "plain", BGRX, "device", "plain"),
         Spec(RGBX, "host", "plain", BGRX64, "host", "bottom-up"),
         Spec(BGRX64, "host", "bottom-up", X2RGB10, "device", "plain"),
         Spec(X2RGB10, "device", "plain", RGBX, "host", "plain"),
         Spec(NV12, "host", "plain", BGRX, "host", "bottom-up"),
         Spec(BGRX, "host", "bottom-up", NV12, "device", "plain"),
         Spec(RGBX, "device", "plain", RGBX, "device", "plain"),
         Spec(BGRX64, "device", "plain", BGRX, "host", "plain"),
         Spec(X2RGB10, "host", "plain", BGRX64, "device", "plain"),
         Spec(BGRX, "host", "plain", X2RGB10, "host", "bottom-up"),
         Spec(NV12, "device", "plain", RGBX, "host", "bottom-up")]
CASES = [(R.ALPHA_SOURCE, F.TRIANGLE), (R.ALPHA_SOURCE, F.CATMULL_ROM), (R.ALPHA_SOURCE, F.MITCHELL), (R.ALPHA_OPAQUE, F.TRIANGLE)]
CASE_IDS = ["source-triangle", "source-catmull-rom", "source-mitchell", "opaque"]


def has_slot(fmt):
    return A.kind_of(fmt) != "none"


def in_planes(fmt, bgrx, seed):
    """(the planes of `bgrx` as a frame of `fmt` with random alpha in its slot, the codes -- None without a slot)."""
    if fmt == NV12:
        h, w = bgrx.shape[:2]
        y = np.ascontiguousarray(bgrx[..., 1])
        uv = np.ascontiguousarray(bgrx[::2, :, 2] // 2 + 64)      # (any chroma: colour is held to the twin fed the same planes)
        assert uv.shape == (h // 2, w)
        return [y, uv], None
    if fmt == BGR24:                                              # (no slot either, and no parity rule: odd sizes)
        return [np.ascontiguousarray(bgrx[..., :3])], None
    arr, codes = with_alpha(fmt, bgrx, seed)
    return [arr], codes


def out_planes(fmt, h, w):
    if fmt == NV12:
        return [np.full((h, w), 0x5A, np.uint8), np.full((h // 2, w), 0x5A, np.uint8)]
    if fmt == BGR24:
        return [np.full((h, w, 3), 0x5A, np.uint8)]
    return [blank(fmt, h, w)]


def make_inputs(specs, clip, seed=700):
    return [in_planes(s.fin, f, seed + t) for t, (s, f) in enumerate(zip(specs, clip))]


def frame_by_frame(blob, dtype, configure, specs, inputs, out_hw):
    """The single-frame route on plain host frames: (every frame's output planes, the state and history, stats)."""
    outs = []
    with R.Runtime(blob, 0, dtype) as rt:
        configure(rt)
        for s, (planes, _) in zip(specs, inputs):
            pout = out_planes(s.fout, *out_hw)
            rt.process_frame(R.host_frame(s.fin, planes), R.host_frame(s.fout, pout))
            outs.append(pout)
        assert rt.stat("lookahead_frames") == 0 and rt.stat("lookahead_alpha_frames") == 0
        return outs, snapshot(rt), {k: rt.stat(k) for k in ("alpha_frames", "scene_cuts")}, rt.scene_info(64)


def check_definition(specs, inputs, got, twin, mode, filt, in_hw, out_hw):
    """The slot is the numpy definition's; colour is the mode-0 twin's, whose slot is 0."""
    for t, (s, (_, codes)) in enumerate(zip(specs, inputs)):
        if not has_slot(s.fout):
            assert all(np.array_equal(x, y) for x, y in zip(got[t], twin[t])), t
            continue
        colour, slot = split(s.fout, got[t][0])
        twin_colour, twin_slot = split(s.fout, twin[t][0])
        want = A.alpha(mode, A.kind_of(s.fin), codes, in_hw, A.kind_of(s.fout), out_hw, filt)
        assert np.array_equal(colour, twin_colour) and (twin_slot == 0).all(), (t, s)
        assert np.array_equal(slot, want), (t, s)


def make_sides(specs, inputs, in_hw, out_hw):
    ins = [Side(s.fin, s.lin, s.layin, planes, in_hw[1], in_hw[0]) for s, (planes, _) in zip(specs, inputs)]
    outs = [Side(s.fout, s.lout, s.layout, out_planes(s.fout, *out_hw), out_hw[1], out_hw[0]) for s in specs]
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def references(blob, dtype, settings, mode, filt, specs, inputs, in_hw, out_hw):
    """(the single-frame route's planes and state under `settings` + the alpha setting, its stats, its records) -- held to
    the definition and to the mode-0 twin on the way."""
    def with_alpha_set(rt):
        settings(rt)
        rt.set_alpha(mode, filt)
    single, snap, stats, records = frame_by_frame(blob, dtype, with_alpha_set, specs, inputs, out_hw)
    twin, twin_snap, _, twin_records = frame_by_frame(blob, dtype, settings, specs, inputs, out_hw)
    check_definition(specs, inputs, single, twin, mode, filt, in_hw, out_hw)
    assert all(np.array_equal(x, y) for x, y in zip(snap, twin_snap)) and records == twin_records
    assert stats["alpha_frames"] == sum(has_slot(s.fout) for s in specs)
    return single, snap, stats, records


@pytest.mark.parametrize("mode,filt", CASES, ids=CASE_IDS)
def test_passes_carry_the_alpha_of_every_format_and_location(mode, filt):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    in_hw, out_hw = (h, w), (4 * h, 4 * w)
    dtype = R.DTYPE_BF16 if filt == F.MITCHELL else R.DTYPE_F16
    clip = M.synthetic_frames(11, h, w, seed=5, kind="smooth")
    inputs = make_inputs(SPECS, clip)
    single, snap, _, _ = references(blob, dtype, lambda rt: None, mode, filt, SPECS, inputs, in_hw, out_hw)
    slots = [has_slot(s.fout) for s in SPECS]
    ins, _ = make_sides(SPECS, inputs, in_hw, out_hw)
    with R.Runtime(blob, 0, dtype) as a:
        a.set_alpha(mode, filt)
        assert a.stat("alpha_lookahead") == 0 and a.stat("lookahead_alpha_frames") == 0
        a.set_alpha_lookahead(1)
        assert a.stat("alpha_lookahead") == 1 and a.get_alpha() == (mode, filt)
        frames = in_pass = written = 0
        for chunks in ((11,), (2, 2, 2, 2, 2, 1)):
            a.reset()
            assert a.stat("alpha_lookahead") == 1                 # (ju_reset keeps the setting)
            _, outs = make_sides(SPECS, inputs, in_hw, out_hw)    # (fresh outputs: every byte is written again)
            run_calls(a, ins, outs, single, chunks)               # (every output byte, guard bytes included)
            assert same_as(a, snap), chunks
            passes = 11 if chunks == (11,) else 10                # (a call of one frame is no pass)
            frames += passes
            in_pass += sum(slots[:passes])
            written += sum(slots)
            assert a.stat("lookahead_frames") == frames and a.stat("lookahead_alpha_frames") == in_pass, chunks
            assert a.stat("alpha_frames") == written, chunks
        assert a.stat("fallbacks") == 0 and a.stat("source_stage_frames") == 0
        for x in ins:
            x.untouched()                                         # (the inputs and their guard bytes: read only)


def test_alpha_goes_from_the_source_size_straight_to_the_output_size_inside_staged_passes():
    cfg = small_config()
    blob = blob_of(cfg)
    in_hw, out_hw = (48, 72), (90, 130)
    specs = SPECS[:7]
    clip = M.synthetic_frames(len(specs), *in_hw, seed=12, kind="smooth")
    inputs = make_inputs(specs, clip, seed=800)
    mask = make_mask((37, 50), 2)

    def settings(rt):
        rt.set_source_size(in_hw[1], in_hw[0], F.MITCHELL)
        rt.set_output_size(out_hw[1], out_hw[0], F.TRIANGLE)
        rt.set_source_mask(mask)
    single, snap, _, _ = references(blob, R.DTYPE_F16, settings, R.ALPHA_SOURCE, F.CATMULL_ROM, specs, inputs, in_hw, out_hw)
    ins, outs = make_sides(specs, inputs, in_hw, out_hw)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        settings(a)
        a.set_alpha(R.ALPHA_SOURCE, F.CATMULL_ROM)
        a.set_alpha_lookahead(1)
        # a runtime under a source size still needs ju_set_stage_lookahead to form passes
        run_calls(a, ins, outs, single, (len(specs),))
        assert a.stat("lookahead_frames") == 0 and a.stat("alpha_frames") == len(specs) - 1 and same_as(a, snap)
        a.set_stage_lookahead(1)
        a.reset()
        _, outs = make_sides(specs, inputs, in_hw, out_hw)
        run_calls(a, ins, outs, single, (len(specs),))
        assert same_as(a, snap)
        assert a.stat("lookahead_frames") == a.stat("lookahead_staged_frames") == len(specs)
        assert a.stat("lookahead_alpha_frames") == len(specs) - 1 and a.stat("alpha_frames") == 2 * (len(specs) - 1)
        for x in ins:
            x.untouched()


def test_a_scene_cut_inside_a_pass_that_carries_alpha():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    in_hw, out_hw = (h, w), (4 * h, 4 * w)
    specs = SPECS[:8]
    first, second = M.synthetic_frames(4, h, w, seed=5, kind="smooth"), M.synthetic_frames(4, h, w, seed=91, kind="smooth")
    clip = list(first) + [255 - f for f in second]               # a cut at frame 4
    inputs = make_inputs(specs, clip, seed=900)

    def settings(rt):
        rt.set_scene_detect(R.SCENE_RESET, 10000)
    single, snap, stats, records = references(blob, R.DTYPE_F16, settings, R.ALPHA_SOURCE, F.TRIANGLE, specs, inputs, in_hw, out_hw)
    cuts = [r["cut"] for r in records]
    assert len(cuts) == 8 and cuts[4] == 1 and not any(cuts[1:4]), cuts   # (the cut lies inside the pass)
    ins, outs = make_sides(specs, inputs, in_hw, out_hw)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        settings(a)
        a.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        a.set_alpha_lookahead(1)
        a.set_scene_lookahead(1)
        run_calls(a, ins, outs, single, (8,))
        assert same_as(a, snap) and a.scene_info(64) == records
        assert a.stat("lookahead_frames") == 8 and a.stat("scene_pass_frames") == 8
        assert a.stat("lookahead_alpha_frames") == a.stat("alpha_frames") == 7


def device_buffers(frames, out_hw):
    """(input tensor [n, H, W, 4], output tensor [n, OH, OW, 4]) on the device."""
    torch, dev = torch_dev()
    d_in = torch.from_numpy(np.stack(frames)).to(dev)
    d_out = torch.full((len(frames),) + out_hw + (4,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return d_in, d_out


def images(rt, d_in, d_out):
    n, h, w = d_in.shape[:3]
    oh, ow = d_out.shape[1:3]
    return ([rt.device_image(d_in[k].data_ptr(), w, h) for k in range(n)],
            [rt.device_image(d_out[k].data_ptr(), ow, oh) for k in range(n)])


def test_setting_changes_between_passes_over_the_same_buffers_leave_no_stale_graph():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    clip = M.synthetic_frames(4, h, w, seed=3, kind="smooth")
    frames = [with_alpha(BGRX, f, 300 + t)[0] for t, f in enumerate(clip)]
    d_in, d_out = device_buffers(frames, (4 * h, 4 * w))
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as s:
        ins, dsts = images(a, d_in, d_out)
        a.set_alpha_lookahead(1)
        # (mode, filter, alpha_lookahead): SOURCE, OPAQUE, ZERO, SOURCE with another filter, the setting off and on again
        steps = [(R.ALPHA_SOURCE, F.TRIANGLE, 1), (R.ALPHA_OPAQUE, F.TRIANGLE, 1), (R.ALPHA_ZERO, F.TRIANGLE, 1),
                 (R.ALPHA_SOURCE, F.MITCHELL, 1), (R.ALPHA_SOURCE, F.MITCHELL, 0), (R.ALPHA_SOURCE, F.MITCHELL, 1),
                 (R.ALPHA_SOURCE, F.TRIANGLE, 1)]
        frames_in_passes = 0
        for mode, filt, on in steps:
            s.set_alpha(mode, filt)
            s.reset()
            want = np.stack([s.process_image(f) for f in frames])  # frame by frame, the single-frame route
            kept = a.stat("alpha_lookahead")
            a.set_alpha(mode, filt)
            assert a.stat("alpha_lookahead") == kept              # (ju_set_alpha keeps the setting)
            a.set_alpha_lookahead(on)
            assert a.stat("alpha_lookahead") == on and a.get_alpha() == (mode, filt)
            for run in range(3):                                  # eager, captured, replayed -- over the same buffers
                a.reset()
                d_out.fill_(0x5A)
                torch.cuda.synchronize()
                a.process_batch(ins, dsts)
                assert np.array_equal(d_out.cpu().numpy(), want), (mode, filt, on, run)
                frames_in_passes += 4 if on or mode == R.ALPHA_ZERO else 0
                assert a.stat("lookahead_frames") == frames_in_passes, (mode, filt, on, run)
        assert np.array_equal(d_in.cpu().numpy(), np.stack(frames))
        # a size setter rebuilds the alpha scaler: the graphs of the passes that carry alpha go with the old tables
        a.reset()
        a.process_batch(ins, dsts)
        a.set_output_size(4 * w, 4 * h, F.TRIANGLE)               # (the model's own output size: the scaler is the identity's)
        a.set_output_size(0, 0)
        s.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        s.reset()
        want = np.stack([s.process_image(f) for f in frames])
        for run in range(3):
            a.reset()
            d_out.fill_(0x5A)
            torch.cuda.synchronize()
            a.process_batch(ins, dsts)
            assert np.array_equal(d_out.cpu().numpy(), want), run


def test_the_same_buffers_again_are_captured_once_and_replayed_and_prepare_batch_captures_as_in_mode_zero():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    clip = M.synthetic_frames(4, h, w, seed=8, kind="smooth")
    frames = [with_alpha(BGRX, f, 600 + t)[0] for t, f in enumerate(clip)]
    d_in, d_out = device_buffers(frames, (4 * h, 4 * w))
    with R.Runtime(blob, 0, R.DTYPE_F16) as s:
        s.set_alpha(R.ALPHA_SOURCE, F.CATMULL_ROM)
        want = np.stack([s.process_image(f) for f in frames])
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        ins, dsts = images(a, d_in, d_out)
        a.set_alpha(R.ALPHA_SOURCE, F.CATMULL_ROM)
        a.set_alpha_lookahead(1)
        seen = []
        for run in range(4):
            a.reset()
            d_out.fill_(0x5A)
            torch.cuda.synchronize()
            a.process_batch(ins, dsts)
            assert np.array_equal(d_out.cpu().numpy(), want), run
            seen.append((a.stat("graph_captures"), a.stat("graph_replays")))
        # an even number of frames: the binding set is the same at every use -- eager, captured, then replayed
        assert seen[1][0] == seen[0][0] + 1 and seen[2][0] == seen[3][0] == seen[1][0]
        assert seen[3][1] > seen[2][1] > seen[0][1] and a.stat("lookahead_alpha_frames") == 16
    with R.Runtime(blob, 0, R.DTYPE_F16) as zero, R.Runtime(blob, 0, R.DTYPE_F16) as a:
        ins, dsts = images(a, d_in, d_out)
        in_mode_zero = zero.prepare_batch(*images(zero, d_in, d_out))
        assert in_mode_zero > 0
        a.set_alpha(R.ALPHA_SOURCE, F.CATMULL_ROM)
        assert a.prepare_batch(ins, dsts) == 0                    # (alpha_lookahead 0: the tuple will not go as one pass)
        a.set_alpha_lookahead(1)
        assert a.prepare_batch(ins, dsts) == in_mode_zero and a.prepare_frames(ins[0], dsts[0]) == 0
        captures, eager = a.stat("graph_captures"), a.stat("eager_runs")
        for run in range(2):
            d_out.fill_(0x5A)
            torch.cuda.synchronize()
            a.process_batch(ins, dsts)
        assert a.stat("graph_captures") == captures and a.stat("graph_replays") >= 2 and a.stat("eager_runs") == eager
        a.reset()
        d_out.fill_(0x5A)
        torch.cuda.synchronize()
        a.process_batch(ins, dsts)
        assert np.array_equal(d_out.cpu().numpy(), want)


def test_a_pass_made_to_run_again_writes_alpha_frame_by_frame():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    in_hw, out_hw = (h, w), (4 * h, 4 * w)
    specs = SPECS[:6]
    clip = M.synthetic_frames(len(specs), h, w, seed=21, kind="smooth")
    inputs = make_inputs(specs, clip, seed=1000)
    single, snap, _, _ = references(blob, R.DTYPE_F16, lambda rt: None, R.ALPHA_SOURCE, F.MITCHELL, specs, inputs, in_hw, out_hw)
    ins, outs = make_sides(specs, inputs, in_hw, out_hw)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        a.set_alpha(R.ALPHA_SOURCE, F.MITCHELL)
        a.set_alpha_lookahead(1)
        assert lib.ju_debug_set(b"pass_rerun", 1) == 0
        try:
            run_calls(a, ins, outs, single, (len(specs),))
        finally:
            lib.ju_debug_set(b"pass_rerun", 0)
        assert same_as(a, snap)
        n = sum(has_slot(s.fout) for s in specs)
        assert a.stat("alpha_frames") == n and a.stat("lookahead_alpha_frames") == 0 and a.stat("lookahead_frames") == 0
        for x in ins:
            x.untouched()


def test_group_members_ride_with_their_own_mode_filter_and_sizes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    src_hw, out_hw = (48, 72), (90, 130)
    mask = make_mask((37, 50), 2)
    # member: (mode, filter, staged, spec)
    members = [(R.ALPHA_SOURCE, F.CATMULL_ROM, False, Spec(BGRX, "device", "plain", BGRX, "device", "plain")),
               (R.ALPHA_OPAQUE, F.TRIANGLE, False, Spec(NV12, "host", "plain", BGRX64, "host", "bottom-up")),
               (R.ALPHA_SOURCE, F.MITCHELL, True, Spec(RGBX, "host", "bottom-up", X2RGB10, "device", "plain")),
               (R.ALPHA_ZERO, F.TRIANGLE, False, Spec(BGRX64, "device", "plain", RGBX, "host", "plain"))]
    ticks = 3

    def settings_of(k):
        mode, filt, staged, _ = members[k]

        def settings(rt):
            if staged:
                rt.set_source_size(src_hw[1], src_hw[0], F.TRIANGLE)
                rt.set_output_size(out_hw[1], out_hw[0], F.CATMULL_ROM)
                rt.set_source_mask(mask)
        return settings

    sizes = [((src_hw, out_hw) if m[2] else ((h, w), (4 * h, 4 * w))) for m in members]
    inputs, singles, snaps = [], [], []
    for k, (mode, filt, staged, spec) in enumerate(members):
        clip = M.synthetic_frames(ticks, *sizes[k][0], seed=40 + k, kind="smooth")
        specs = [spec] * ticks
        inputs.append(make_inputs(specs, clip, seed=1100 + 10 * k))
        if mode == R.ALPHA_ZERO:                                  # the plain member: the frame-by-frame route in mode 0
            single, snap, _, _ = frame_by_frame(blob, R.DTYPE_F16, settings_of(k), specs, inputs[k], sizes[k][1])
        else:                                                     # that member run alone, held to the definition and the twin
            single, snap, _, _ = references(blob, R.DTYPE_F16, settings_of(k), mode, filt, specs, inputs[k], *sizes[k])
        singles.append(single)
        snaps.append(snap)
    rts = [R.Runtime(blob, 0, R.DTYPE_F16) for _ in members]
    try:
        for k, (mode, filt, staged, _) in enumerate(members):
            settings_of(k)(rts[k])
            rts[k].set_alpha(mode, filt)
            assert rts[k].stat("alpha_group") == 0
            rts[k].set_alpha_group(1)
            if staged:
                rts[k].set_stage_group(1)
            assert rts[k].stat("alpha_group") == 1 and rts[k].stat("alpha_lookahead") == 0
        for t in range(ticks):
            sides = [make_sides([m[3]], [inputs[k][t]], *sizes[k]) for k, m in enumerate(members)]
            R.process_group_frames(rts, [s[0][0].frame for s in sides], [s[1][0].frame for s in sides])
            for k, s in enumerate(sides):
                s[1][0].check(singles[k][t])                      # (every member's frame equals that member run alone)
                s[0][0].untouched()
        for k, (mode, filt, staged, spec) in enumerate(members):
            assert same_as(rts[k], snaps[k]), k
            assert rts[k].stat("group_frames") == ticks, k         # (all four ride)
            rides = ticks if mode != R.ALPHA_ZERO and has_slot(spec.fout) else 0
            assert rts[k].stat("group_alpha_frames") == rides and rts[k].stat("alpha_frames") == rides, k
            assert rts[k].stat("group_staged_frames") == (ticks if staged else 0) and rts[k].stat("lookahead_alpha_frames") == 0
        # with the setting off the member runs alone behind the pass, the others still ride
        rts[0].set_alpha_group(0)
        sides = [make_sides([m[3]], [inputs[k][0]], *sizes[k]) for k, m in enumerate(members)]
        R.process_group_frames(rts, [s[0][0].frame for s in sides], [s[1][0].frame for s in sides])
        assert rts[0].stat("group_frames") == ticks and rts[1].stat("group_frames") == ticks + 1
        assert rts[0].stat("alpha_frames") == ticks + 1 and rts[0].stat("group_alpha_frames") == ticks
    finally:
        for rt in rts:
            rt.close()


def test_defaults_and_refusals():
    cfg = small_config()
    blob = blob_of(cfg)
    lib = R.load_library(True)
    keys = ("alpha_lookahead", "alpha_group", "lookahead_alpha_frames", "group_alpha_frames", "alpha_frames", "alpha_mode")
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        assert all(a.stat(k) == 0 for k in keys)
        for name, setter, key in (("ju_set_alpha_lookahead", a.set_alpha_lookahead, "alpha_lookahead"),
                                  ("ju_set_alpha_group", a.set_alpha_group, "alpha_group")):
            for start in (0, 1):
                setter(start)
                before = {k: a.stat(k) for k in keys}
                for bad in (2, -1, 255):
                    with pytest.raises(R.JoshUpscaleError, match=name):
                        setter(bad)
                    assert getattr(lib, name)(a._h, bad) == 1       # (the C layer itself)
                    assert lib.ju_last_error().decode() == f"std::invalid_argument: {name}: on must be 0 or 1, got {bad}"
                    assert {k: a.stat(k) for k in keys} == before
            setter(0)
        # ju_set_alpha and ju_reset keep both
        a.set_alpha_lookahead(1)
        a.set_alpha_group(1)
        a.set_alpha(R.ALPHA_OPAQUE)
        a.reset()
        a.set_alpha(R.ALPHA_ZERO)
        assert a.stat("alpha_lookahead") == 1 and a.stat("alpha_group") == 1
