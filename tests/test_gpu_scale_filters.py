"""The cubic filters of the source and the output scaler on the GPU (csrc/source_kernels.hip, the signed forms of
scale_bgrx_kernel and scale_state_kernel; docs/source_stage.md "Filters"): each kernel alone against the numpy definition
(tests/scale_filter_reference.py), byte for byte with the guard bytes around every row; runtimes with a filter set
against a twin whose frames are scaled in numpy; every entry point; the refused calls."""

import numpy as np
import pytest

import output_reference as O
import scale_filter_reference as F
import source_reference as S
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_output import SIZES, blank, byte_rows, out_frame, result, same_planes, state_content, twin_record
from test_gpu_source import LAYOUTS, SRC_H, SRC_W, frame_of, make_mask, read_back, same_state
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import decoded, source, state_of

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
BGRX, NV12, P010 = R.FMT_BGRX, R.FMT_NV12, R.FMT_P010
CUBIC = pytest.mark.parametrize("filt", F.CUBIC, ids=lambda f: F.NAMES[f])

# (source, destination) as (H, W): down, almost equal, up (one-tap rows between four-tap rows), equal, a source that ends
# inside a quad, and 4 : 1 across 15 tiles (the bank padding of the tile)
SCALE_CASES = [((30, 46), (16, 24)), ((17, 23), (16, 24)), ((8, 12), (16, 24)), ((16, 24), (16, 24)), ((33, 49), (16, 24)),
               ((64, 1920), (16, 480))]
# 8 : 1 on both axes (32-tap rows, the widest tile span), 1 : 16 (one source pixel under 16 outputs), both at once
LIMIT_CASES = [((64, 1024), (8, 128)), ((4, 6), (64, 96)), ((96, 40), (12, 640))]
STATE_CASES = [((16, 24), (12, 18)), ((16, 24), (24, 36)), ((16, 24), (16, 24)), ((16, 24), (7, 50)), ((17, 23), (16, 24))]


def debug_scale(op, filt, dst_ptr, dst_stride, dst_hw, src_ptr, src_stride, src_hw):
    lib = R.load_library(True)
    rc = lib.ju_debug_scale(op, filt, dst_ptr, dst_stride, dst_hw[1], dst_hw[0], src_ptr, src_stride, src_hw[1], src_hw[0],
                            None, None, None)
    assert rc == 0, lib.ju_last_error()


# ---- 1. scale_bgrx_kernel, signed ------------------------------------------------------------------------------------------
_REF8 = {}


def scale_case(src_hw, dst_hw, kind, filt):
    """(source, numpy result) of one case, computed once for all layouts."""
    key = (src_hw, dst_hw, kind, filt)
    if key not in _REF8:
        h, w = src_hw
        if kind == "random":
            src = np.random.default_rng(h * 131 + w).integers(0, 256, (h, w, 4), dtype=np.uint8)   # (X random: ignored)
        elif kind == "edges":
            src = F.step_edges(h, w)
            src[..., 3] = 0xC3
        else:
            src = np.full((h, w, 4), 0 if kind == "zero" else 255, np.uint8)
        _REF8[key] = (src, F.scale8(src, *dst_hw, filt))
    return _REF8[key]


@CUBIC
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_scale_kernel_equals_the_numpy_definition(layout, filt):
    lay = LAYOUTS[layout]
    clamped = False
    for src_hw, dst_hw in SCALE_CASES:
        for kind in ("random", "zero", "full", "edges"):
            src, want = scale_case(src_hw, dst_hw, kind, filt)
            d_src = DevPlane(src, **lay)
            d_dst = DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **lay)
            debug_scale(0, filt, d_dst.ptr, d_dst.stride, dst_hw, d_src.ptr, d_src.stride, src_hw)
            d_dst.check(want)                                   # (and the guard bytes around every row)
            d_src.check(src)                                    # (the source untouched)
            if kind in ("zero", "full"):
                assert (want[..., :3] == (0 if kind == "zero" else 255)).all()
            if kind == "edges" and src_hw != dst_hw:
                raw = F.sums(src, *dst_hw, filt)[1] >> 24
                clamped |= int(raw.min()) < 0 and int(raw.max()) > 255
            if src_hw == dst_hw:                                # N = M: Catmull-Rom is the identity, Mitchell is not
                assert np.array_equal(want[..., :3], src[..., :3]) == (filt == F.CATMULL_ROM or kind in ("zero", "full"))
    assert clamped                                              # (the clamp worked at both ends)


@CUBIC
def test_scale_kernel_at_the_ratio_limits(filt):
    rng = np.random.default_rng(3)
    most = 0
    for src_hw, dst_hw in LIMIT_CASES:
        src = rng.integers(0, 256, src_hw + (4,), dtype=np.uint8)
        d_src, d_dst = DevPlane(src, pad=16), DevPlane(np.zeros(dst_hw + (4,), np.uint8), pad=4, offset=4)
        debug_scale(0, filt, d_dst.ptr, d_dst.stride, dst_hw, d_src.ptr, d_src.stride, src_hw)
        d_dst.check(F.scale8(src, *dst_hw, filt))
        most = max(most, *(int(F.axis_table(n, m, filt)[1].max()) for n, m in zip(src_hw, dst_hw)))
    assert most == 32


# ---- 2. scale_state_kernel, signed -----------------------------------------------------------------------------------------
def state_of_kind(kind, h, w):
    if kind != "edges":
        return state_content(kind, h, w)
    p = F.step_edges(h, w, 65535, np.int64)                               # an f16 step edge: P = 0 / 65535 exactly
    s = np.where(p == 0, np.float16(-0.5), np.float16(0.5)).astype(np.float16)
    assert np.array_equal(O.p_from_state(s), p[..., :3])
    return s


@CUBIC
@pytest.mark.parametrize("kind", ["random", "low", "high", "beyond", "edges"])
def test_scale_state_kernel_equals_the_numpy_definition(kind, filt):
    for src_hw, dst_hw in STATE_CASES:
        state = state_of_kind(kind, *src_hw)
        p = O.p_from_state(state)
        want = F.scale16(p, *dst_hw, filt)
        if kind == "low":
            assert (p == 0).all() and (want == 0).all()
        if kind == "high":
            assert (p == 65535).all() and (want[..., :3] == 65535).all()
        if kind == "beyond":
            assert (p == 0).any() and (p == 65535).any()
        if kind == "edges" and dst_hw == (24, 36):
            raw = F.sums(p, *dst_hw, filt)[1] >> 24
            assert int(raw.min()) < 0 and int(raw.max()) > 65535 and int(want.max()) == 65535   # (the clamp, both ends)
        if src_hw == dst_hw and filt == F.CATMULL_ROM:
            assert np.array_equal(want[..., :3], p)
        d_src = DevPlane(byte_rows(state))
        d_dst = DevPlane(np.full((dst_hw[0], dst_hw[1] * 8), 0x5A, np.uint8))
        assert d_src.ptr % 16 == 0 and d_dst.ptr % 8 == 0
        debug_scale(1, filt, d_dst.ptr, 0, dst_hw, d_src.ptr, 0, src_hw)
        d_dst.check(byte_rows(want))                                      # (and the guard bytes around the frame)
        d_src.check(byte_rows(state))


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
def blob_of(**kw):
    cfg = small_config(**kw)
    return cfg, M.serialize(cfg, M.make_seeded_weights(cfg))


@CUBIC
def test_a_scaled_source_equals_the_twin_fed_the_numpy_scale(filt):
    cfg, blob = blob_of()
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(4, SRC_H, SRC_W, seed=5, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert a.stat("source_filter") == 0
        a.set_source_size(SRC_W, SRC_H, filt)
        assert a.get_source_size() == (SRC_W, SRC_H) and a.stat("source_filter") == filt and a.stat("output_filter") == 0
        for t, f in enumerate(clip):
            fmt, location = ((BGRX, "host"), (NV12, "device"), (BGRX, "device"), (NV12, "host"))[t]
            keep = []
            planes = source(f, fmt, CS)
            small = F.scale8(decoded(fmt, CS, planes), h, w, filt)
            assert not np.array_equal(small, S.scale(decoded(fmt, CS, planes), h, w))
            want = b.process_image(small)
            out = blank(BGRX, 4 * h, 4 * w)
            a.process_frame(frame_of(fmt, planes, location, keep), frame_of(BGRX, out, location, keep))
            got = out[0] if location == "host" else read_back(BGRX, out, keep[-1])[0]
            assert np.array_equal(got, want), t
        assert same_state(a, b)
        a.reset()                                                         # (keeps the size and the filter)
        b.reset()
        assert a.get_source_size() == (SRC_W, SRC_H) and a.stat("source_filter") == filt
        assert np.array_equal(a.process_image(clip[0]), b.process_image(F.scale8(clip[0], h, w, filt)))
        a.set_source_size(0, 0)
        assert a.stat("source_filter") == 0 and a.stat("source_scaled") == 0


@CUBIC
def test_outputs_equal_the_twins_frame_and_state_scaled_in_numpy(filt):
    cfg, blob = blob_of()
    clip = M.synthetic_frames(2, cfg.frame_height, cfg.frame_width, seed=5, kind="smooth")
    rec = twin_record(blob, clip)
    eight, sixteen = (BGRX, NV12, R.FMT_RGB24), (P010, R.FMT_BGRX64, R.FMT_RGBPH)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        assert a.stat("output_filter") == 0
        for (oh, ow) in SIZES:
            a.set_output_size(ow, oh, filt)
            assert a.get_output_size() == (ow, oh) and a.stat("output_filter") == filt and a.stat("source_filter") == 0
            want8 = [F.scale8(r[0], oh, ow, filt) for r in rec]
            want16 = [F.scale16(O.p_from_state(r[1]), oh, ow, filt) for r in rec]
            assert not np.array_equal(want8[0], O.scale8(rec[0][0], oh, ow))
            for k, fmt in enumerate(eight + sixteen):
                a.reset()                                                 # (keeps the size and the filter)
                assert a.get_output_size() == (ow, oh) and a.stat("output_filter") == filt
                for t, f in enumerate(clip):
                    location = ("host", "device")[(t + k) % 2]
                    if fmt == BGRX:
                        want = [want8[t]]
                    else:
                        want = O.encode8(fmt, CS, want8[t]) if fmt in eight else O.encode16(fmt, CS, want16[t])
                    planes = blank(fmt, oh, ow)
                    keep = []
                    a.process_frame(R.host_frame(BGRX, [f]), out_frame(fmt, planes, ow, oh, location, keep))
                    assert same_planes(result(planes, location, keep), want), (fmt, (oh, ow), t, location)
                    assert np.array_equal(a.read_tensor("state"), rec[t][2]), (fmt, t)      # the unscaled twin's
                    assert np.array_equal(a.read_tensor("flow_in"), rec[t][3]), (fmt, t)
        a.set_output_size(0, 0)
        assert a.stat("output_filter") == 0 and a.stat("output_scaled") == 0


@pytest.mark.parametrize("src_filt,out_filt", [(F.CATMULL_ROM, F.MITCHELL), (F.MITCHELL, F.TRIANGLE), (F.TRIANGLE, F.CATMULL_ROM)],
                         ids=lambda f: F.NAMES[f])
def test_a_source_size_a_mask_and_an_output_size_with_different_filters(src_filt, out_filt):
    cfg, blob = blob_of()
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(3, SRC_H, SRC_W, seed=9, kind="smooth")
    mask = make_mask((37, 50), 2)
    oh, ow = SIZES[0]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H, src_filt)
        a.set_source_mask(mask)
        a.set_output_size(ow, oh, out_filt)
        assert (a.stat("source_filter"), a.stat("output_filter")) == (src_filt, out_filt)
        for t, f in enumerate(clip):
            fmt, out_fmt = (NV12, BGRX, BGRX)[t], (BGRX, P010, NV12)[t]
            planes = source(f, fmt, CS)
            src = decoded(fmt, CS, planes)
            plain = b.process_image(F.scale8(src, h, w, src_filt) if src_filt else S.scale(src, h, w))
            blended = S.blend(plain, src, mask)
            want8 = F.scale8(blended, oh, ow, out_filt) if out_filt else O.scale8(blended, oh, ow)
            want = [want8] if out_fmt == BGRX else O.encode8(out_fmt, CS, want8)    # (masked: deep formats from the 8-bit frame)
            got = blank(out_fmt, oh, ow)
            a.process_frame(R.host_frame(fmt, planes, CS), R.host_frame(out_fmt, got, CS))
            assert same_planes(got, want), t
            assert same_state(a, b), t
        # without the mask a P010 output comes from the scaled state again
        a.set_source_mask(None)
        planes = source(clip[0], BGRX, CS)
        b.process_image(F.scale8(clip[0], h, w, src_filt) if src_filt else S.scale(clip[0], h, w))
        p = O.p_from_state(state_of(b, h, w))
        want = O.encode16(P010, CS, F.scale16(p, oh, ow, out_filt) if out_filt else O.scale16(p, oh, ow))
        got = blank(P010, oh, ow)
        a.process_frame(R.host_frame(BGRX, planes, CS), R.host_frame(P010, got, CS))
        assert same_planes(got, want)


def test_every_entry_point_gives_the_frames_of_process_image():
    filt = F.CATMULL_ROM
    cfg, blob = blob_of()
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = SIZES[1]
    clip = M.synthetic_frames(8, SRC_H, SRC_W, seed=21, kind="smooth")
    torch, dev = torch_dev()
    members = [R.Runtime(blob, 0, R.DTYPE_F16) for _ in range(2)]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b, R.Runtime(blob, 0, R.DTYPE_F16) as plain:
        try:
            for rt in [a, b] + members:
                rt.set_source_size(SRC_W, SRC_H, filt)
                rt.set_output_size(ow, oh, filt)
            want = [b.process_image(f).copy() for f in clip]              # process_image: ju_process on host frames
            # ... which is the numpy scale of the twin's frame of the numpy-scaled source
            assert np.array_equal(want[0], F.scale8(plain.process_image(F.scale8(clip[0], h, w, filt)), oh, ow, filt))
            # ju_process, device frames
            d_in = torch.from_numpy(np.stack(clip)).to(dev)
            d_out = torch.zeros((len(clip), oh, ow, 4), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            img = lambda rt, k: (rt.device_image(d_in[k].data_ptr(), SRC_W, SRC_H), rt.device_image(d_out[k].data_ptr(), ow, oh))
            a.process(*img(a, 0))
            # ju_process_frame, host frames
            out = blank(BGRX, oh, ow)
            a.process_frame(R.host_frame(BGRX, [clip[1]]), R.host_frame(BGRX, out))
            assert np.array_equal(out[0], want[1])
            # ju_process_batch, 4 device frames
            pairs = [img(a, k) for k in range(2, 6)]
            a.process_batch([p[0] for p in pairs], [p[1] for p in pairs])
            got = d_out.cpu().numpy()
            for k in (0, 2, 3, 4, 5):
                assert np.array_equal(got[k], want[k]), k
            # ju_process_group: two members, every one the whole stream from its start
            for k in range(2):
                R.process_group(members, [img(members[0], k)[0]] * 2, [members[0].device_image(d_out[6 + j].data_ptr(), ow, oh) for j in range(2)])
                got = d_out.cpu().numpy()
                assert np.array_equal(got[6], want[k]) and np.array_equal(got[7], want[k]), k
            for k in (6, 7):                                              # (a catches up with b: the states agree too)
                assert np.array_equal(a.process_image(clip[k]), want[k])
            assert same_state(a, b)
            for rt in [a] + members:
                assert rt.stat("lookahead_frames") == 0 and rt.stat("group_frames") == 0
        finally:
            for rt in members:
                rt.close()


def test_refused_calls_leave_the_size_the_filter_and_the_bytes_as_they_were():
    cfg, blob = blob_of()
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = SIZES[0]
    clip = M.synthetic_frames(3, SRC_H, SRC_W, seed=30, kind="smooth")
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        for rt in (a, b):
            rt.set_source_size(SRC_W, SRC_H, F.MITCHELL)
            rt.set_output_size(ow, oh, F.CATMULL_ROM)
        assert np.array_equal(a.process_image(clip[0]), b.process_image(clip[0]))
        # filter 1, filter 4, and 9 : 1 with a cubic filter (8 : 1 at most), on either stage: the Python twin and the C call
        bad_source = [(SRC_W, SRC_H, 1), (SRC_W, SRC_H, 4), (9 * w, SRC_H, F.CATMULL_ROM), (SRC_W, 9 * h, F.MITCHELL), (0, 0, 1)]
        bad_output = [(ow, oh, 1), (ow, oh, 4), (4 * w // 9, oh, F.CATMULL_ROM), (ow, 4 * h // 9, F.MITCHELL), (0, 0, 1)]
        for setter, c_call, cases in ((a.set_source_size, lib.ju_set_source_size, bad_source),
                                      (a.set_output_size, lib.ju_set_output_size, bad_output)):
            for (sw, sh, filt) in cases:
                with pytest.raises(ValueError) as e:
                    setter(sw, sh, filt)
                assert c_call(a._h, sw, sh, filt) == 1
                assert lib.ju_last_error().decode() == "std::invalid_argument: " + str(e.value)
                assert ("filter" in str(e.value)) == (filt in (1, 4)) and ("8 times" in str(e.value) or "8th" in str(e.value)) == (filt not in (1, 4))
        # 9 : 1 is the triangle's to take (16 : 1 at most) -- on a third runtime, a stays as it was
        with R.Runtime(blob, 0, R.DTYPE_F16) as c:
            c.set_source_size(9 * w, SRC_H, F.TRIANGLE)
            c.set_output_size(4 * w // 9, oh)
        assert a.get_source_size() == (SRC_W, SRC_H) and a.get_output_size() == (ow, oh)
        assert (a.stat("source_filter"), a.stat("output_filter")) == (F.MITCHELL, F.CATMULL_ROM)
        for f in clip[1:]:
            assert np.array_equal(a.process_image(f), b.process_image(f))
        assert same_state(a, b)
