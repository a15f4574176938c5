"""The output stage on the GPU (csrc/source_kernels.hip scale_state_kernel, csrc/colour_kernels.hip Bgrx16Source,
engine_frames.cpp "Output stage"; docs/output_stage.md): the 16-bit scaler and the encode from a 16-bit frame alone against the
numpy definition (tests/output_reference.py), byte for byte; a runtime with an output size set against a twin whose
frame and state are scaled and encoded in numpy; with a source size and a mask; models whose deep outputs come from the
8-bit frame; every entry point; turning it off; the refused calls."""

import ctypes as C

import numpy as np
import pytest

import output_reference as O
import source_reference as S
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_source import make_mask, same_state
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import decoded, source, state_of

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
BGRX, NV12, I420, P010, I010 = R.FMT_BGRX, R.FMT_NV12, R.FMT_I420, R.FMT_P010, R.FMT_I010
SIZES = [(90, 144), (180, 288)]                                  # (OH, OW) for the 120 x 192 frames of the small model
EIGHT = (BGRX, NV12, I420, R.FMT_YUY2, R.FMT_RGB24)
SIXTEEN = (P010, I010, R.FMT_I410, R.FMT_BGRX64, R.FMT_RGBPH, R.FMT_RGBPS)
NAMES = {BGRX: "bgrx", **O.NAMES}


def byte_rows(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def same_planes(got, want):
    return len(got) == len(want) and all(g.dtype == e.dtype and g.shape == e.shape and
                                         np.array_equal(byte_rows(g), byte_rows(e)) for g, e in zip(got, want))


def blank(fmt, h, w):
    if fmt == BGRX:
        return [np.zeros((h, w, 4), np.uint8)]
    return O.G.blank_planes(fmt, h, w) if fmt in O.G.NEW_FORMATS else O.YS.blank_planes(fmt, h, w)


def debug_output(op, dst, dst_hw, src, src_hw=(0, 0), fmt=0, cs=0, planes=()):
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    return lib.ju_debug_output(op, dst, dst_hw[1], dst_hw[0], src, src_hw[1], src_hw[0], fmt, cs, ptrs, strides)


# ---- 1. scale_state_kernel alone ----------------------------------------------------------------------------------------
# (state size, output size) as (H, W): down, up, the identity, both at once; an odd width (rows at 8-byte alignment);
# the ratio limits 16 : 1 (33 taps, the widest tile span, two tiles across) and 1 : 16
STATE_CASES = [((16, 24), (12, 18)), ((16, 24), (24, 36)), ((16, 24), (16, 24)), ((16, 24), (7, 50)), ((17, 23), (16, 24)),
               ((64, 1024), (4, 64)), ((4, 6), (64, 96))]


def state_content(kind, h, w):
    rng = np.random.default_rng(h * 977 + w)
    if kind == "random":
        return rng.uniform(-0.5, 0.5, (h, w, 4)).astype(np.float16)       # (the fourth value: ignored)
    if kind == "low":
        return np.full((h, w, 4), -0.5, np.float16)
    if kind == "high":
        return np.full((h, w, 4), 0.5, np.float16)                        # (65536: saturates at 65535)
    s = rng.uniform(-0.5, 0.5, (h, w, 4)).astype(np.float16)              # "beyond": a few samples that saturate
    flat = s.reshape(-1)
    where = rng.choice(flat.size, max(flat.size // 16, 4), replace=False)
    flat[where[0::2]] = -1.0
    flat[where[1::2]] = 0.75
    return s


@pytest.mark.parametrize("kind", ["random", "low", "high", "beyond"])
def test_scale_state_kernel_equals_the_numpy_definition(kind):
    for src_hw, dst_hw in STATE_CASES:
        state = state_content(kind, *src_hw)
        p = O.p_from_state(state)
        want = O.scale16(p, *dst_hw)
        if kind == "low":
            assert (p == 0).all() and (want == 0).all()
        if kind == "high":
            assert (p == 65535).all() and (want[..., :3] == 65535).all()
        if kind == "beyond":
            assert (p == 0).any() and (p == 65535).any()
        if src_hw == dst_hw:
            assert np.array_equal(want[..., :3], p)                       # N = M: the identity
        d_src = DevPlane(byte_rows(state))
        d_dst = DevPlane(np.full((dst_hw[0], dst_hw[1] * 8), 0x5A, np.uint8))
        assert d_src.ptr % 16 == 0 and d_dst.ptr % 8 == 0
        rc = debug_output(0, d_dst.ptr, dst_hw, d_src.ptr, src_hw)
        assert rc == 0, R.load_library(True).ju_last_error()
        d_dst.check(byte_rows(want))                                      # (and the guard bytes around the frame)
        d_src.check(byte_rows(state))                                     # (the source untouched)


# ---- 2. the encode from a 16-bit frame ----------------------------------------------------------------------------------
ENCODE_LAYOUTS = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=32, offset=0, flip=False),
                  "bottom-up": dict(pad=16, offset=0, flip=True)}
_FRAME16 = {}


def frame16(h, w):
    if (h, w) not in _FRAME16:
        rng = np.random.default_rng(41)
        p = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)            # (X random: ignored)
        p[0, :4, :3], p[1, :4, :3] = 0, 65535                             # (both ends of the range, at every size)
        if h > 2 and w > 2:
            p[2, 0, :3], p[2, 1, :3], p[2, 2, :3] = (0, 65535, 0), (65535, 0, 65535), (1, 63, 64)
        _FRAME16[(h, w)] = p
    return _FRAME16[(h, w)]


@pytest.mark.parametrize("layout", sorted(ENCODE_LAYOUTS))
@pytest.mark.parametrize("fmt", O.DEEP, ids=lambda f: NAMES[f])
def test_encode_from_a_16_bit_frame_equals_the_numpy_definition(fmt, layout):
    lay = ENCODE_LAYOUTS[layout]
    for (h, w) in [(16, 24), (2, 2), (6, 34)]:                            # (one strip and a half, the smallest, three strips)
        p = frame16(h, w)
        d_src = DevPlane(byte_rows(p))
        for cs in ((0, 1, 2, 3) if fmt in O.DEEP_YUV and (h, w) == (16, 24) else (CS,)):
            want = O.encode16(fmt, cs, p)
            planes = [DevPlane(np.full_like(byte_rows(e), 0x5A), **lay) for e in want]
            rc = debug_output(1, None, (h, w), d_src.ptr, fmt=fmt, cs=cs, planes=planes)
            assert rc == 0, R.load_library(True).ju_last_error()
            for d, e in zip(planes, want):
                d.check(byte_rows(e))
        d_src.check(byte_rows(p))


def test_encode_from_a_16_bit_frame_refuses_8_bit_formats():
    lib = R.load_library(True)
    p = frame16(16, 24)
    d_src = DevPlane(byte_rows(p))
    for fmt in (NV12, I420, R.FMT_YUY2, R.FMT_I444, R.FMT_RGB24, R.FMT_RGBP8, BGRX, 99):
        planes = [DevPlane(np.full((16, 24 * 4), 0x5A, np.uint8)) for _ in range(3)]
        assert debug_output(1, None, (16, 24), d_src.ptr, fmt=fmt, cs=CS, planes=planes) == 1
        assert b"deep" in lib.ju_last_error()
        for d in planes:
            d.check(np.full((16, 24 * 4), 0x5A, np.uint8))


# ---- 3. end to end -------------------------------------------------------------------------------------------------------
def blob_and_clip(n, seed=5, **kw):
    cfg = small_config(**kw)
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    return cfg, blob, M.synthetic_frames(n, cfg.frame_height, cfg.frame_width, seed=seed, kind="smooth")


def out_frame(fmt, planes, w, h, location, keep, cs=CS):
    """A ju_frame over output planes: host arrays as they are (any row order), or dense device copies kept in `keep`."""
    if location == "host":
        keep.append(planes)
        if fmt == BGRX:
            return R.host_frame(BGRX, planes)
        return R.host_frame(fmt, planes, cs)
    torch, dev = torch_dev()
    held = [torch.from_numpy(byte_rows(p)).to(dev) for p in planes]
    torch.cuda.synchronize()
    keep.append(held)
    return R.device_frame(fmt, w, h, held, [t.shape[1] for t in held], cs)


def result(planes, location, keep):
    if location == "host":
        return planes
    return [t.cpu().numpy().view(p.dtype).reshape(p.shape) for t, p in zip(keep[-1], planes)]


def twin_record(blob, clip, dtype=R.DTYPE_F16):
    """Per frame of the clip what a runtime without an output size leaves: (frame, f16 state, the two state tensors)."""
    rec = []
    with R.Runtime(blob, 0, dtype) as b:
        h, w = b.input_height, b.input_width
        for f in clip:
            frame = b.process_image(f).copy()
            rec.append((frame, state_of(b, h, w), b.read_tensor("state").copy(), b.read_tensor("flow_in").copy()))
    return rec


def test_outputs_equal_the_twins_frame_and_state_scaled_in_numpy():
    cfg, blob, clip = blob_and_clip(4)
    rec = twin_record(blob, clip)
    frames = 0
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        assert a.get_output_size() == (0, 0) and a.stat("output_scaled") == 0 and a.stat("hbd_from_state") == 1
        for (oh, ow) in SIZES:
            a.set_output_size(ow, oh)
            assert a.get_output_size() == (ow, oh) and a.stat("output_scaled") == 1
            assert (a.output_width, a.output_height) == (4 * cfg.frame_width, 4 * cfg.frame_height)   # (ju_get_size: the model's)
            want8 = [O.scale8(r[0], oh, ow) for r in rec]
            want16 = [O.scale16(O.p_from_state(r[1]), oh, ow) for r in rec]
            for k, fmt in enumerate(EIGHT + SIXTEEN):
                a.reset()                                                 # (keeps the setting)
                assert a.get_output_size() == (ow, oh)
                for t, f in enumerate(clip):
                    location = ("host", "device")[(t + k) % 2]
                    if fmt == BGRX:
                        want = [want8[t]]
                    else:
                        want = O.encode8(fmt, CS, want8[t]) if fmt in EIGHT else O.encode16(fmt, CS, want16[t])
                    assert O.takes_16_bit_path(fmt, True, False) == (fmt in SIXTEEN)
                    planes = blank(fmt, oh, ow)
                    flip = location == "host" and t == 1                  # a bottom-up host output
                    keep = []
                    a.process_frame(R.host_frame(BGRX, [f]),
                                    out_frame(fmt, [p[::-1] for p in planes] if flip else planes, ow, oh, location, keep))
                    got = result(planes, location, keep)
                    if flip:
                        got = [p[::-1] for p in got]
                    assert same_planes(got, want), (NAMES[fmt], (oh, ow), t, location)
                    assert np.array_equal(a.read_tensor("state"), rec[t][2]), (NAMES[fmt], t)
                    assert np.array_equal(a.read_tensor("flow_in"), rec[t][3]), (NAMES[fmt], t)
                    frames += 1
        assert a.stat("lookahead_frames") == 0 and a.stat("source_stage_frames") == frames
        # Runtime.process_image allocates at the output size
        a.reset()
        oh, ow = SIZES[-1]
        assert np.array_equal(a.process_image(clip[0]), O.scale8(rec[0][0], oh, ow))


# ---- 4. with a source size and a mask ------------------------------------------------------------------------------------
def test_a_source_size_a_mask_and_an_output_size_together():
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(3, 48, 72, seed=9, kind="smooth")
    mask = make_mask((37, 50), 2)
    oh, ow = SIZES[0]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(72, 48)
        a.set_source_mask(mask)
        a.set_output_size(ow, oh)
        assert a.stat("hbd_from_state") == 1                              # (the model's property; the mask decides the path)
        for t, f in enumerate(clip):
            fmt = (NV12, BGRX, I420)[t]
            planes = source(f, fmt, CS)
            src = decoded(fmt, CS, planes)
            plain = b.process_image(S.scale(src, h, w))
            blended = S.blend(plain, src, mask)
            assert (blended != plain).any()
            want8 = O.scale8(blended, oh, ow)
            out_fmt = (BGRX, P010, NV12)[t]
            got = blank(out_fmt, oh, ow)
            a.process_frame(R.host_frame(fmt, planes, CS), R.host_frame(out_fmt, got, CS))
            want = O.output(out_fmt, CS, oh, ow, blended, state_of(b, h, w), hbd_from_state=True, masked=True)
            if out_fmt == P010:
                assert same_planes(want, O.encode8(P010, CS, want8))      # the 257 u8 encode of the scaled blend
            assert same_planes(got, want), t
            assert same_state(a, b), t                                    # neither the blend nor the scale feeds back
        assert a.stat("source_stage_frames") == 3


# ---- 5. which frame a deep output comes from -----------------------------------------------------------------------------
def test_a_pre_warp_models_deep_outputs_come_from_the_scaled_8_bit_frame():
    cfg, blob, clip = blob_and_clip(4, seed=11, output="pre_warp")
    oh, ow = SIZES[1]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert a.output == "pre_warp" and a.stat("hbd_from_state") == 0
        a.set_output_size(ow, oh)
        for t, f in enumerate(clip):
            fmt = (P010, R.FMT_BGRX64, R.FMT_RGBPS, R.FMT_I410)[t]
            got = blank(fmt, oh, ow)
            a.process_frame(R.host_frame(BGRX, [f]), R.host_frame(fmt, got, CS))
            frame = b.process_image(f)
            want = O.output(fmt, CS, oh, ow, frame, None, hbd_from_state=False)
            assert same_planes(want, O.encode8(fmt, CS, O.scale8(frame, oh, ow)))
            assert same_planes(got, want), (NAMES[fmt], t)
            assert same_state(a, b), t


def test_a_flow_free_models_p010_output_comes_from_its_state():
    """A flow-free model has no readable state; its twin's BGRX64 output at model size IS the state's P (W16 = P), and
    from that the scaled P010 follows."""
    cfg = small_config()
    cfg, wts = M.remove_flow(cfg, M.make_seeded_weights(cfg))
    blob = M.serialize(cfg, wts)
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = SIZES[0]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert not a.recurrent and a.stat("hbd_from_state") == 1
        a.set_output_size(ow, oh)
        for t, f in enumerate(M.synthetic_frames(2, h, w, seed=6, kind="smooth")):
            p = blank(R.FMT_BGRX64, 4 * h, 4 * w)
            b.process_frame(R.host_frame(BGRX, [f]), R.host_frame(R.FMT_BGRX64, p))
            want = O.encode16(P010, CS, O.scale16(p[0], oh, ow))
            got = blank(P010, oh, ow)
            a.process_frame(R.host_frame(BGRX, [f]), R.host_frame(P010, got, CS))
            assert same_planes(got, want), t
            assert len(np.unique((got[0] >> 6) % 4)) == 4                 # (all of the two extra bits in use)


# ---- 6. every entry point --------------------------------------------------------------------------------------------------
def test_every_entry_point_hands_out_the_scaled_frame():
    cfg, blob, clip = blob_and_clip(15, seed=21)
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = SIZES[0]
    torch, dev = torch_dev()
    want_of = lambda rt, f: O.scale8(rt.process_image(f), oh, ow)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_output_size(ow, oh)
        # ju_process, host
        assert np.array_equal(a.process_image(clip[0]), want_of(b, clip[0]))
        # ju_process_batch, 5 device frames
        d_in = torch.from_numpy(np.stack(clip[1:6])).to(dev)
        d_out = torch.zeros((5, oh, ow, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        a.process_batch([a.device_image(d_in[k].data_ptr(), w, h) for k in range(5)],
                        [a.device_image(d_out[k].data_ptr(), ow, oh) for k in range(5)])
        got = d_out.cpu().numpy()
        for k in range(5):
            assert np.array_equal(got[k], want_of(b, clip[1 + k])), k
        # ju_process_frames, 3 host NV12 frames -> NV12
        outs = [blank(NV12, oh, ow) for _ in range(3)]
        planes = [source(f, NV12, CS) for f in clip[6:9]]
        a.process_frames([R.host_frame(NV12, p, CS) for p in planes], [R.host_frame(NV12, o, CS) for o in outs])
        for k in range(3):
            assert same_planes(outs[k], O.encode8(NV12, CS, want_of(b, decoded(NV12, CS, planes[k])))), k
        # ju_enqueue + ju_synchronize, device frames
        for k in range(2):
            a.enqueue(a.device_image(d_in[k].data_ptr(), w, h), a.device_image(d_out[k].data_ptr(), ow, oh))
        a.synchronize()
        got = d_out.cpu().numpy()
        for k in range(2):
            assert np.array_equal(got[k], want_of(b, clip[1 + k])), k
        assert same_state(a, b)
        assert a.stat("lookahead_frames") == 0 and a.stat("group_frames") == 0 and a.stat("source_stage_frames") == 11
        # ju_prepare_* capture nothing
        assert a.prepare_frames(a.device_image(d_in[0].data_ptr(), w, h), a.device_image(d_out[0].data_ptr(), ow, oh)) == 0
        assert a.prepare_batch([a.device_image(d_in[k].data_ptr(), w, h) for k in range(3)],
                               [a.device_image(d_out[k].data_ptr(), ow, oh) for k in range(3)]) == 0
        # off again: a look-ahead pass and the plain bytes, on the same runtime
        a.set_output_size(0, 0)
        assert a.get_output_size() == (0, 0) and a.stat("output_scaled") == 0
        s_in = torch.from_numpy(np.stack(clip[9:13])).to(dev)
        p_out = torch.zeros((4, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        a.process_batch([a.device_image(s_in[k].data_ptr(), w, h) for k in range(4)],
                        [a.device_image(p_out[k].data_ptr(), 4 * w, 4 * h) for k in range(4)])
        got = p_out.cpu().numpy()
        for k in range(4):
            assert np.array_equal(got[k], b.process_image(clip[9 + k])), k
        assert a.stat("lookahead_frames") == 4 and a.stat("source_stage_frames") == 11
        assert same_state(a, b)


def test_a_group_with_an_output_size_runs_member_by_member():
    cfg, blob, clip = blob_and_clip(2, seed=4)
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = SIZES[1]
    torch, dev = torch_dev()
    members = [R.Runtime(blob, 0, R.DTYPE_F16) for _ in range(3)]
    twin = R.Runtime(blob, 0, R.DTYPE_F16)
    try:
        for rt in members:
            rt.set_output_size(ow, oh)
        d_out = torch.zeros((3, oh, ow, 4), dtype=torch.uint8, device=dev)
        for t, f in enumerate(clip):                              # (every member sees the same stream: one twin serves all)
            d_in = torch.from_numpy(np.stack([f] * 3)).to(dev)
            torch.cuda.synchronize()
            R.process_group(members, [members[0].device_image(d_in[k].data_ptr(), w, h) for k in range(3)],
                            [members[0].device_image(d_out[k].data_ptr(), ow, oh) for k in range(3)])
            want = O.scale8(twin.process_image(f), oh, ow)
            got = d_out.cpu().numpy()
            for k in range(3):
                assert np.array_equal(got[k], want), (t, k)
        for rt in members:
            assert same_state(rt, twin)
            assert rt.stat("group_frames") == 0 and rt.stat("lookahead_frames") == 0 and rt.stat("source_stage_frames") == 2
    finally:
        for rt in members + [twin]:
            rt.close()


# ---- 7. refused calls ------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_runtime_as_it_was():
    cfg, blob, clip = blob_and_clip(3, seed=30)
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = SIZES[0]
    torch, dev = torch_dev()
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_output_size(ow, oh)
        assert np.array_equal(a.process_image(clip[0]), O.scale8(b.process_image(clip[0]), oh, ow))
        big = np.zeros((4 * h, 4 * w, 4), np.uint8)
        out = np.zeros((oh, ow, 4), np.uint8)

        def refused(call, words):
            with pytest.raises(R.JoshUpscaleError) as e:
                call()
            assert e.value.code == 1 and words in e.value.message, e.value.message

        # a model-size output while an output size is set, on each kind of entry point
        named = f"exactly {ow}x{oh} (the output size set)"
        refused(lambda: a.process(R.host_image(clip[1]), R.host_image(big)), named)
        refused(lambda: a.process_batch([R.host_image(clip[1])] * 2, [R.host_image(out), R.host_image(big)]), "frame 1")
        refused(lambda: a.process_frame(R.host_frame(BGRX, [clip[1]]), R.host_frame(BGRX, [big])), named)
        refused(lambda: R.process_group([a], [R.host_image(clip[1])], [R.host_image(big)]), named)
        refused(lambda: a.process_frame(R.host_frame(BGRX, [clip[1]]), R.host_frame(NV12, blank(NV12, 4 * h, 4 * w), CS)), named)
        # an axis beyond a factor of 16, an axis of 1, an unknown filter: the Python twin and the C call, with one message
        for (sw, sh, filt) in [(16 * 4 * w + 1, oh, 0), (ow, 4 * h // 16 - 1, 0), (ow, 1, 0), (1, oh, 0), (ow, oh, 1)]:
            with pytest.raises(ValueError) as e:
                a.set_output_size(sw, sh, filt)
            assert lib.ju_set_output_size(a._h, sw, sh, filt) == 1
            assert lib.ju_last_error().decode() == "std::invalid_argument: " + str(e.value)
        assert b"filter" in lib.ju_last_error()
        assert a.get_output_size() == (ow, oh)
        # an odd output size with an NV12 output
        a.set_output_size(ow + 1, oh + 1)
        odd = [np.zeros((oh + 1, ow + 1), np.uint8), np.zeros((oh // 2, ow + 1), np.uint8)]
        fr = R.host_frame(NV12, odd, CS)
        refused(lambda: a.process_frame(R.host_frame(BGRX, [clip[1]]), fr), "even")
        a.set_output_size(ow, oh)
        # a graphics resource as the output
        tex = torch.zeros((oh, ow * 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        try:
            assert lib.ju_debug_fake_gl_texture(22, tex.data_ptr(), ow * 4, ow, oh, 4) == 0
            img = R.gl_image(22, output=True)
            refused(lambda: a.process(R.host_image(clip[1]), img), "graphics resources cannot be outputs")
            refused(lambda: R.process_group([a], [R.host_image(clip[1])], [img]), "graphics resources cannot be outputs")
            R.release_gl_image(img)
        finally:
            lib.ju_debug_fake_gl_texture(0, None, 0, 0, 0, 0)
        assert a.stat("source_stage_frames") == 1
        # nothing ran: the stream goes on as its twin's
        for f in clip[1:]:
            assert np.array_equal(a.process_image(f), O.scale8(b.process_image(f), oh, ow))
        assert same_state(a, b)
