"""Alpha on a tiled object (ju_tiled_set_alpha; tiled.cpp; docs/tiled.md "Alpha").  Byte for byte, no tolerance: the slot
equals the numpy definition (tests/alpha_reference.py) from the tiled source size straight to the output frame's size;
every colour byte equals a second tiled object in mode 0 fed the same frames -- unscaled and under an output size, under
a mask, with deep outputs from the 8-bit frame and from the states, across a reset; look-ahead passes equal frame by
frame; a one-tile object equals a plain runtime under ju_set_alpha; the refusals change nothing; mode 0 again is an
object that never had the setting."""

import dataclasses

import numpy as np
import pytest

import alpha_reference as A
import scale_filter_reference as F
from helpers import M
from joshupscale_amd import runtime as R
from test_gpu_alpha import BGRX, RGBX
from test_gpu_alpha_passes import BGR24, SPECS, check_definition, has_slot, make_inputs, make_sides, out_planes
from test_gpu_source import make_mask
from test_gpu_tiled_deep import small_blob
from test_tiled_output_cpu import GEOMETRIES, H, W

pytestmark = pytest.mark.gpu

NINE, FOUR, ONE = GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[4]    # (100, 70, 4), (49, 31, 7), (48, 30, 7)


def specs_for(sw, sh, order):
    """The passes' specs; a source of odd size cannot be NV12, so its format without a slot is BGR24."""
    specs = [SPECS[k] for k in order]
    if sw % 2 or sh % 2:
        specs = [dataclasses.replace(s, fin=BGR24 if s.fin == R.FMT_NV12 else s.fin, fout=BGR24 if s.fout == R.FMT_NV12 else s.fout)
                 for s in specs]
    return specs


def even_size(sw, sh):
    """An output size (h, w), even on both axes, about one and a half times the source and no multiple of it."""
    return 2 * (sh + sh // 2) - 2, 2 * (sw + sw // 2) + 2


def clip_of(sw, sh, n, seed=5):
    return M.synthetic_frames(n, sh, sw, seed=seed, kind="smooth")


def run_frames(tr, specs, inputs, in_hw, out_hw, reset_at=None):
    """Frame by frame through ju_tiled_process_frame at the specs' formats and locations: every frame's output planes,
    guard bytes checked to be whole, the inputs untouched."""
    got = []
    for t, s in enumerate(specs):
        if t == reset_at:
            tr.reset()
        ins, outs = make_sides([s], [inputs[t]], in_hw, out_hw)
        tr.process_frame(ins[0].frame, outs[0].frame)
        ins[0].untouched()
        planes = [np.array(p._rows(p.buf.cpu().numpy() if hasattr(p, "buf") else p.host)) for p in outs[0].planes]
        outs[0].check(planes)                                     # (nothing but the rows was written)
        shaped = [p.view(o.dtype).reshape(o.shape) for p, o in zip(planes, out_planes(s.fout, *out_hw))]
        got.append(shaped)
    return got


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geometry", [NINE, FOUR], ids=["nine-tiles", "four-tiles"])
def test_a_tiled_object_carries_alpha_and_leaves_colour_to_its_mode_zero_twin(geometry, dtype):
    sw, sh, ov = geometry
    blob = small_blob()
    in_hw = (sh, sw)
    filt = F.CATMULL_ROM if dtype == R.DTYPE_F16 else F.MITCHELL
    order = list(range(7)) if dtype == R.DTYPE_F16 else [7, 8, 9, 10, 0, 3, 5]
    specs = specs_for(sw, sh, order)
    clip = clip_of(sw, sh, 7)
    inputs = make_inputs(specs, clip, seed=1300)
    mask = make_mask((37, 50), 2)
    odd = even_size(sw, sh)
    with R.TiledRuntime(blob, 0, dtype, sw, sh, ov) as a, R.TiledRuntime(blob, 0, dtype, sw, sh, ov) as b:
        assert a.get_alpha() == (0, 0) and a.stat("alpha_mode") == 0 and a.stat("alpha_frames") == 0
        written = 0
        # (mode, output size, mask, deep_from_state)
        phases = [(R.ALPHA_SOURCE, None, False, 0), (R.ALPHA_SOURCE, odd, True, 0), (R.ALPHA_SOURCE, odd, False, 1),
                  (R.ALPHA_OPAQUE, None, True, 1)]
        for mode, size, masked, deep in phases:
            out_hw = size or (4 * sh, 4 * sw)
            for tr in (a, b):
                tr.reset()
                tr.set_output_size(*((size[1], size[0]) if size else (0, 0)), F.TRIANGLE)
                tr.set_source_mask(mask if masked else None)
                tr.set_deep_from_state(deep)
            a.set_alpha(mode, filt)
            assert a.get_alpha() == (mode, filt) and a.stat("alpha_mode") == mode and a.stat("alpha_filter") == filt
            got = run_frames(a, specs, inputs, in_hw, out_hw, reset_at=4)     # four frames, a reset, three more
            assert a.get_alpha() == (mode, filt)                              # (ju_tiled_reset keeps the setting)
            twin = run_frames(b, specs, inputs, in_hw, out_hw, reset_at=4)
            check_definition(specs, inputs, got, twin, mode, filt, in_hw, out_hw)
            written += sum(has_slot(s.fout) for s in specs)
            assert a.stat("alpha_frames") == written and b.stat("alpha_frames") == 0
            for key in ("frames", "group_frames", "deep_state_frames", "output_scaled_frames", "source_mask_frames"):
                assert a.stat(key) == b.stat(key), key
        # mode 0 again: the bytes of the object that never had the setting, slot included
        a.set_alpha(R.ALPHA_ZERO, filt)
        for tr in (a, b):
            tr.reset()
        got = run_frames(a, specs[:3], inputs[:3], in_hw, out_hw)
        twin = run_frames(b, specs[:3], inputs[:3], in_hw, out_hw)
        assert all(np.array_equal(x, y) for g, t in zip(got, twin) for x, y in zip(g, t))
        assert a.stat("alpha_frames") == written


def test_process_frames_passes_equal_frame_by_frame():
    sw, sh, ov = FOUR
    blob = small_blob()
    in_hw, out_hw = (sh, sw), even_size(sw, sh)
    specs = specs_for(sw, sh, range(7))
    inputs = make_inputs(specs, clip_of(sw, sh, 7, seed=9), seed=1400)
    mask = make_mask((37, 50), 2)

    def settings(tr):
        tr.set_output_size(out_hw[1], out_hw[0], F.MITCHELL)
        tr.set_source_mask(mask)
        tr.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as b:
        settings(a)
        settings(b)
        want = run_frames(b, specs, inputs, in_hw, out_hw)
        for chunks in ((7,), (3, 4)):
            a.reset()
            ins, outs = make_sides(specs, inputs, in_hw, out_hw)
            t = 0
            for k in chunks:
                a.process_frames([x.frame for x in ins[t:t + k]], [x.frame for x in outs[t:t + k]])
                t += k
            for i in range(7):
                outs[i].check(want[i])                            # (every output byte, guard bytes included)
                ins[i].untouched()
        assert a.stat("pass_frames") == 14 and a.stat("alpha_frames") == 2 * b.stat("alpha_frames") == 12


def test_an_output_size_set_under_source_rebuilds_the_alpha_scaler():
    """ju_tiled_set_output_size under SOURCE, with no ju_tiled_set_alpha behind it: the alpha goes to the new size."""
    sw, sh, ov = FOUR
    blob = small_blob()
    in_hw = (sh, sw)
    specs = specs_for(sw, sh, [0, 1, 3])
    inputs = make_inputs(specs, clip_of(sw, sh, 3, seed=4), seed=1600)
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as b:
        a.set_alpha(R.ALPHA_SOURCE, F.CATMULL_ROM)
        for size in (even_size(sw, sh), None, (2 * sh, 6 * sw)):      # an output size, none again, another one
            out_hw = size or (4 * sh, 4 * sw)
            for tr in (a, b):
                tr.reset()
                tr.set_output_size(*((size[1], size[0]) if size else (0, 0)), F.MITCHELL)
            assert a.get_alpha() == (R.ALPHA_SOURCE, F.CATMULL_ROM)   # (ju_tiled_set_output_size keeps the setting)
            got = run_frames(a, specs, inputs, in_hw, out_hw)
            twin = run_frames(b, specs, inputs, in_hw, out_hw)
            check_definition(specs, inputs, got, twin, R.ALPHA_SOURCE, F.CATMULL_ROM, in_hw, out_hw)
        assert a.stat("alpha_frames") == 9


def test_a_one_tile_object_equals_a_plain_runtime_under_ju_set_alpha():
    sw, sh, ov = ONE
    assert (sw, sh) == (W, H)
    blob = small_blob()
    in_hw, out_hw = (sh, sw), (4 * sh, 4 * sw)
    specs = [SPECS[0], SPECS[1], SPECS[3], SPECS[9]]
    inputs = make_inputs(specs, clip_of(sw, sh, 4, seed=2), seed=1500)
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as a, R.Runtime(blob, 0, R.DTYPE_F16) as rt:
        assert a.stat("tiles") == 1
        a.set_deep_from_state(1)                                  # (a plain runtime encodes a deep format from its state)
        a.set_alpha(R.ALPHA_SOURCE, F.MITCHELL)
        rt.set_alpha(R.ALPHA_SOURCE, F.MITCHELL)
        got = run_frames(a, specs, inputs, in_hw, out_hw)
        for t, s in enumerate(specs):
            pout = out_planes(s.fout, *out_hw)
            rt.process_frame(R.host_frame(s.fin, inputs[t][0]), R.host_frame(s.fout, pout))
            assert all(np.array_equal(x, y) for x, y in zip(got[t], pout)), t


def test_the_refused_calls_change_nothing():
    sw, sh, ov = FOUR
    blob = small_blob()
    lib = R.load_library(True)
    keys = ("alpha_mode", "alpha_filter", "alpha_frames", "frames", "output_scaled", "output_filter")
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as a:
        a.set_alpha(R.ALPHA_OPAQUE, F.CATMULL_ROM)
        frame = np.zeros((sh, sw, 4), np.uint8)
        assert (a.run(frame)[..., 3] == 255).all()

        def state():
            return a.get_alpha(), a.get_output_size(), {k: a.stat(k) for k in keys}
        keep = state()
        for mode, filt in [(3, 0), (-1, 0), (R.ALPHA_SOURCE, 1), (R.ALPHA_ZERO, 4)]:
            with pytest.raises(ValueError, match="ju_tiled_set_alpha"):
                a.set_alpha(mode, filt)
            assert lib.ju_tiled_set_alpha(a._h, mode, filt) == 1     # (the C layer itself)
            assert lib.ju_last_error().decode() == "std::invalid_argument: ju_tiled_set_alpha: " + \
                R.tiled_alpha_problem(mode, filt, sw, sh)
            assert state() == keep
        # SOURCE pushed outside the limits: 20 times the source is within the output size's limits (16 times the blended
        # frame), but the alpha scaler goes straight from the source and enlarges 16 times at the most
        big = (20 * sw, 20 * sh)
        text = R.tiled_alpha_problem(R.ALPHA_SOURCE, F.TRIANGLE, sw, sh, *big)
        assert text and "alpha" in text and f"{sw}x{sh}" in text and f"{big[0]}x{big[1]}" in text
        assert not R.tiled_output_size_problem(big[0], big[1], sw, sh, F.TRIANGLE)
        # ... by ju_tiled_set_output_size: alpha is there first
        a.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        keep = state()
        with pytest.raises(ValueError, match="ju_tiled_set_output_size: alpha from the source"):
            a.set_output_size(*big)
        assert lib.ju_tiled_set_output_size(a._h, big[0], big[1], F.TRIANGLE) == 1
        assert lib.ju_last_error().decode() == "std::invalid_argument: ju_tiled_set_output_size: " + text and state() == keep
        # ... by ju_tiled_set_alpha: the output size is there first
        a.set_alpha(R.ALPHA_OPAQUE, F.TRIANGLE)
        a.set_output_size(*big)
        keep = state()
        with pytest.raises(ValueError, match="ju_tiled_set_alpha: alpha from the source"):
            a.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        assert lib.ju_tiled_set_alpha(a._h, R.ALPHA_SOURCE, F.TRIANGLE) == 1
        assert lib.ju_last_error().decode() == "std::invalid_argument: ju_tiled_set_alpha: " + text and state() == keep
        # ... and turning the output size off is fine here (four times the source), after which SOURCE may be set
        a.set_output_size(0, 0)
        a.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        out = a.run(np.full((sh, sw, 4), 200, np.uint8))
        assert (out[..., 3] == 200).all() and a.stat("alpha_frames") == 2 and a.stat("frames") == 2
        # a format without a slot on the output side: nothing launched, nothing counted
        planes = out_planes(R.FMT_NV12, 4 * sh, 4 * sw)
        a.process_frame(R.host_frame(BGRX, [frame]), R.host_frame(R.FMT_NV12, planes))
        assert a.stat("alpha_frames") == 2 and a.stat("frames") == 3
        assert RGBX != BGRX and A.kind_of(R.FMT_NV12) == "none"
