"""The source stage on the GPU (csrc/source_kernels.hip, engine_frames.cpp "Source stage"; docs/source_stage.md): the scale and
the blend kernel alone against the numpy definition (tests/source_reference.py), byte for byte; a runtime with a source
size set against a twin fed scale(decode(source)) computed in numpy; the mask against the numpy blend of the twin's
outputs, and the state against the unmasked twin's; every entry point; turning the settings off; the refused calls."""

import ctypes as C

import numpy as np
import pytest

import source_reference as S
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import BGRX, I010, I420, NAMES, NV12, P010, TEN, as_bytes, blank_planes, decoded, expect_planes, source

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
SRC_H, SRC_W = 48, 72            # the end-to-end source, for the 30 x 48 model: 1.6 and 1.5 to one

# BGRX rows: pad in bytes behind each row, first row `offset` bytes off a 64-byte boundary
LAYOUTS = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=128, offset=0, flip=False),
           "bottom-up": dict(pad=64, offset=0, flip=True), "odd-offset": dict(pad=13, offset=1, flip=False),
           "word-offset": dict(pad=4, offset=4, flip=False)}
SCALE_CASES = [((30, 46), (16, 24)), ((17, 23), (16, 24)), ((8, 12), (16, 24)), ((16, 24), (16, 24)), ((256, 384), (16, 24)),
               ((33, 49), (16, 24)), ((64, 1920), (16, 480))]


def debug_source(op, dst, dst_hw, src, src_hw, mask=None, mask_hw=(0, 0)):
    lib = R.load_library(True)
    rc = lib.ju_debug_source(op, dst.ptr, dst.stride, dst_hw[1], dst_hw[0], src.ptr, src.stride, src_hw[1], src_hw[0],
                             mask.ptr if mask else None, mask.stride if mask else 0, mask_hw[1], mask_hw[0])
    assert rc == 0, lib.ju_last_error()


_SCALE_REF = {}


def scale_case(src_hw, dst_hw, kind):
    """(source, numpy result) of one case, computed once for all layouts."""
    key = (src_hw, dst_hw, kind)
    if key not in _SCALE_REF:
        h, w = src_hw
        if kind == "random":
            src = np.random.default_rng(h * 131 + w).integers(0, 256, (h, w, 4), dtype=np.uint8)   # (X random: ignored)
        else:
            src = np.full((h, w, 4), 0 if kind == "zero" else 255, np.uint8)
        _SCALE_REF[key] = (src, S.scale(src, *dst_hw))
    return _SCALE_REF[key]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_scale_kernel_equals_the_numpy_definition(layout):
    lay = LAYOUTS[layout]
    for src_hw, dst_hw in SCALE_CASES:
        for kind in ("random", "zero", "full"):
            src, want = scale_case(src_hw, dst_hw, kind)
            d_src = DevPlane(src, **lay)
            d_dst = DevPlane(np.full(dst_hw + (4,), 0x5A, np.uint8), **lay)
            debug_source(0, d_dst, dst_hw, d_src, src_hw)
            d_dst.check(want)                                   # (and the guard bytes around every row)
            d_src.check(src)                                    # (the source untouched)
            if src_hw == dst_hw:
                assert np.array_equal(want[..., :3], src[..., :3])   # N = M: the identity


def test_scale_kernel_at_the_ratio_limits():
    """16 to 1 and 1 to 16 on both axes: 33-tap rows, the widest tile span, and one source pixel under 16 outputs."""
    rng = np.random.default_rng(3)
    for src_hw, dst_hw in [((64, 1024), (4, 64)), ((4, 6), (64, 96)), ((96, 40), (6, 640))]:
        src = rng.integers(0, 256, src_hw + (4,), dtype=np.uint8)
        d_src, d_dst = DevPlane(src, pad=16), DevPlane(np.zeros(dst_hw + (4,), np.uint8), pad=4, offset=4)
        debug_source(0, d_dst, dst_hw, d_src, src_hw)
        d_dst.check(S.scale(src, *dst_hw))


@pytest.mark.parametrize("layout", ["dense", "bottom-up", "odd-offset"])
def test_blend_kernel_equals_the_numpy_definition(layout):
    lay = LAYOUTS[layout]
    rng = np.random.default_rng(17)
    oh, ow = 120, 192
    for mask_hw in [(oh, ow), (oh // 2, ow // 2), (37, 50)]:                # output size, half size, no divisor
        for src_hw in [(30, 48), (90, 144)]:                               # model size, 3 x model size
            gen = rng.integers(0, 256, (oh, ow, 4), dtype=np.uint8)        # (X random: kept where the mask is white)
            src = rng.integers(0, 256, src_hw + (4,), dtype=np.uint8)
            mask = rng.integers(0, 256, mask_hw + (4,), dtype=np.uint8)
            kind = rng.integers(0, 3, mask_hw)
            mask[kind == 0, :3] = 255                                      # a third white, a third black, a third anything
            mask[kind == 1, :3] = 0
            want = S.blend(gen, src, mask)
            assert (want == gen).all(-1).any() and (want != gen).any()
            d_gen, d_src, d_mask = DevPlane(gen, **lay), DevPlane(src, **lay), DevPlane(mask, **lay)
            debug_source(1, d_gen, (oh, ow), d_src, src_hw, d_mask, mask_hw)
            d_gen.check(want)
            d_src.check(src)
            d_mask.check(mask)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def blob_and_clip(n, seed=5):
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    return cfg, blob, M.synthetic_frames(n, SRC_H, SRC_W, seed=seed, kind="smooth")


def rows(planes):
    return [as_bytes(p) if p.ndim == 2 else p.reshape(p.shape[0], -1) for p in planes]


def frame_of(fmt, planes, location, keep):
    """A ju_frame over the planes: host arrays as they are, or dense device copies (kept alive in `keep`)."""
    h, w = planes[0].shape[:2]
    if location == "host":
        keep.append(planes)
        return R.host_frame(fmt, planes, CS)
    torch, dev = torch_dev()
    held = [torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in rows(planes)]
    torch.cuda.synchronize()
    keep.append(held)
    return R.device_frame(fmt, w, h, held, [t.shape[1] for t in held], CS)


def read_back(fmt, planes, held):
    """The planes a device frame of frame_of holds now, in the shapes and types of `planes`."""
    return [t.cpu().numpy().view(p.dtype).reshape(p.shape) for t, p in zip(held, planes)]


def same_state(a, b):
    return np.array_equal(a.read_tensor("state"), b.read_tensor("state")) and \
        np.array_equal(a.read_tensor("flow_in"), b.read_tensor("flow_in"))


@pytest.mark.parametrize("fmt", [BGRX, NV12, I420, P010, I010], ids=lambda f: NAMES[f])
def test_a_scaled_source_equals_the_twin_fed_the_numpy_scale(fmt):
    cfg, blob, clip = blob_and_clip(4)
    h, w = cfg.frame_height, cfg.frame_width
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        assert a.get_source_size() == (SRC_W, SRC_H) and b.get_source_size() == (0, 0)
        assert (a.input_width, a.input_height) == (w, h) and a.stat("source_scaled") == 1 and a.stat("source_mask") == 0
        frames = 0
        for location in ("host", "device"):
            for t, f in enumerate(clip):
                keep = []
                planes = source(f, fmt, CS)
                want = b.process_image(S.scale(decoded(fmt, CS, planes), h, w))
                out = blank_planes(BGRX, 4 * h, 4 * w)
                a.process_frame(frame_of(fmt, planes, location, keep), frame_of(BGRX, out, location, keep))
                got = out[0] if location == "host" else read_back(BGRX, out, keep[-1])[0]
                assert np.array_equal(got, want), (location, t)
                frames += 1
            assert same_state(a, b)
        assert a.stat("source_stage_frames") == frames and a.stat("lookahead_frames") == 0


def make_mask(hw, seed):
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 256, hw + (4,), dtype=np.uint8)
    kind = rng.integers(0, 3, hw)
    mask[kind == 0, :3] = 255
    mask[kind == 1, :3] = 0
    return mask


def test_the_mask_blends_the_output_and_never_feeds_back():
    cfg, blob, clip = blob_and_clip(4, seed=9)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    mask = make_mask((37, 50), 2)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b, R.Runtime(blob, 0, R.DTYPE_F16) as c:
        a.set_source_size(SRC_W, SRC_H)
        a.set_source_mask(mask)
        # c: the mask alone, given as a bottom-up device image: the source is the model-size input frame
        held = torch.from_numpy(np.ascontiguousarray(mask[::-1])).to(dev)
        torch.cuda.synchronize()
        c.set_source_mask(R.JuImage(held.data_ptr() + 36 * 200, R.LOC_DEVICE, -200, 50, 37))
        del held                                                  # (the call copied it)
        assert a.stat("source_mask") == 1 and c.stat("source_mask") == 1 and c.stat("source_scaled") == 0
        assert a.stat("hbd_from_state") == 1                      # (the model's property, mask or not)
        for t, f in enumerate(clip):
            fmt = (NV12, BGRX, I010, I420)[t]
            planes = source(f, fmt, CS)
            src = decoded(fmt, CS, planes)
            small = S.scale(src, h, w)
            plain = b.process_image(small)
            want = S.blend(plain, src, mask)
            assert (want != plain).any()
            keep = []
            if t < 3:
                got = blank_planes(BGRX, 4 * h, 4 * w)
                a.process_frame(frame_of(fmt, planes, "host", keep), R.host_frame(R.FMT_BGRX, got))
                assert np.array_equal(got[0], want), t
            else:                                                 # a P010 output: the encode of the blended 8-bit frame
                got = blank_planes(P010, 4 * h, 4 * w)
                a.process_frame(frame_of(fmt, planes, "host", keep), R.host_frame(R.FMT_P010, got, CS))
                for g, e in zip(got, expect_planes(P010, CS, want, None)):
                    assert np.array_equal(g, e)
            assert np.array_equal(c.process_image(small), S.blend(plain, small, mask)), t
        assert same_state(a, b) and same_state(c, b)              # the blend never feeds back
        assert a.stat("source_stage_frames") == 4 and c.stat("source_stage_frames") == 4
        # without the mask the P010 output comes from the f16 state again
        a.set_source_mask(None)
        assert a.stat("source_mask") == 0
        planes = source(clip[0], NV12, CS)
        b.process_image(S.scale(decoded(NV12, CS, planes), h, w))
        got = blank_planes(P010, 4 * h, 4 * w)
        a.process_frame(R.host_frame(NV12, planes, CS), R.host_frame(R.FMT_P010, got, CS))
        state = b.read_tensor("state").reshape(4 * h, 4 * w, 4).astype(np.float16)
        for g, e in zip(got, expect_planes(P010, CS, None, state)):
            assert np.array_equal(g, e)


def test_every_entry_point_runs_the_source_stage_frame_by_frame():
    cfg, blob, clip = blob_and_clip(13, seed=21)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    want_of = lambda rt, f: rt.process_image(S.scale(f, h, w)).copy()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        # ju_process, host
        assert np.array_equal(a.process_image(clip[0]), want_of(b, clip[0]))
        # ju_process_batch, 5 device frames
        d_in = torch.from_numpy(np.stack(clip[1:6])).to(dev)
        d_out = torch.zeros((5, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        a.process_batch([a.device_image(d_in[k].data_ptr(), SRC_W, SRC_H) for k in range(5)],
                        [a.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(5)])
        got = d_out.cpu().numpy()
        for k in range(5):
            assert np.array_equal(got[k], want_of(b, clip[1 + k])), k
        # ju_process_frames, 3 host NV12 frames
        keep, outs = [], [blank_planes(BGRX, 4 * h, 4 * w) for _ in range(3)]
        planes = [source(f, NV12, CS) for f in clip[6:9]]
        a.process_frames([frame_of(NV12, p, "host", keep) for p in planes], [R.host_frame(R.FMT_BGRX, o) for o in outs])
        for k in range(3):
            assert np.array_equal(outs[k][0], want_of(b, decoded(NV12, CS, planes[k]))), k
        # ju_enqueue + ju_synchronize, device frames
        for k in range(2):
            a.enqueue(a.device_image(d_in[k].data_ptr(), SRC_W, SRC_H), a.device_image(d_out[k].data_ptr(), 4 * w, 4 * h))
        a.synchronize()
        got = d_out.cpu().numpy()
        for k in range(2):
            assert np.array_equal(got[k], want_of(b, clip[1 + k])), k
        assert same_state(a, b)
        assert a.stat("lookahead_frames") == 0 and a.stat("source_stage_frames") == 11
        # ju_reset keeps the setting
        a.reset()
        b.reset()
        assert a.get_source_size() == (SRC_W, SRC_H)
        assert np.array_equal(a.process_image(clip[9]), want_of(b, clip[9]))
        # both settings off: look-ahead passes and the plain bytes again, on the same runtime
        a.set_source_size(0, 0)
        a.set_source_mask(None)
        assert a.get_source_size() == (0, 0) and a.stat("source_scaled") == 0
        small = np.stack([S.scale(f, h, w) for f in clip[9:13]])
        s_in = torch.from_numpy(small).to(dev)
        torch.cuda.synchronize()
        a.process_batch([a.device_image(s_in[k].data_ptr(), w, h) for k in range(4)],
                        [a.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(4)])
        got = d_out.cpu().numpy()
        for k in range(4):
            assert np.array_equal(got[k], b.process_image(small[k])), k
        assert a.stat("lookahead_frames") == 4 and a.stat("source_stage_frames") == 12
        assert same_state(a, b)


def test_a_group_of_scaled_runtimes_runs_member_by_member():
    cfg, blob, clip = blob_and_clip(2, seed=4)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    members = [R.Runtime(blob, 0, R.DTYPE_F16) for _ in range(3)]
    twin = R.Runtime(blob, 0, R.DTYPE_F16)
    try:
        for rt in members:
            rt.set_source_size(SRC_W, SRC_H)
        d_out = torch.zeros((3, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        for t, f in enumerate(clip):                              # (every member sees the same stream: one twin serves all)
            d_in = torch.from_numpy(np.stack([f] * 3)).to(dev)
            torch.cuda.synchronize()
            R.process_group(members, [members[0].device_image(d_in[k].data_ptr(), SRC_W, SRC_H) for k in range(3)],
                            [members[0].device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(3)])
            want = twin.process_image(S.scale(f, h, w))
            got = d_out.cpu().numpy()
            for k in range(3):
                assert np.array_equal(got[k], want), (t, k)
        for rt in members:
            assert same_state(rt, twin)
            assert rt.stat("group_frames") == 0 and rt.stat("lookahead_frames") == 0 and rt.stat("source_stage_frames") == 2
    finally:
        for rt in members + [twin]:
            rt.close()


def test_refused_calls_leave_the_runtime_as_it_was():
    cfg, blob, clip = blob_and_clip(3, seed=30)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        assert np.array_equal(a.process_image(clip[0]), b.process_image(S.scale(clip[0], h, w)))
        out = np.zeros((4 * h, 4 * w, 4), np.uint8)

        def refused(call, words):
            with pytest.raises(R.JoshUpscaleError) as e:
                call()
            assert e.value.code == 1 and words in e.value.message, e.value.message

        # a model-size frame while a source size is set, on each kind of entry point
        small = S.scale(clip[1], h, w)
        refused(lambda: a.process(R.host_image(small), R.host_image(out)), "exactly 72x48")
        refused(lambda: a.process_batch([R.host_image(clip[1]), R.host_image(small)], [R.host_image(out)] * 2), "frame 1")
        refused(lambda: a.process_frame(R.host_frame(R.FMT_BGRX, [small]), R.host_frame(R.FMT_BGRX, [out])), "exactly 72x48")
        refused(lambda: R.process_group([a], [R.host_image(small)], [R.host_image(out)]), "exactly 72x48")
        # ratios beyond 16, an axis below 2, an unknown filter: the Python twin and the C call, with one message
        for (sw, sh) in [(16 * w + 1, SRC_H), (SRC_W, 1), (2, SRC_H)]:
            with pytest.raises(ValueError) as e:
                a.set_source_size(sw, sh)
            assert lib.ju_set_source_size(a._h, sw, sh, 0) == 1
            assert lib.ju_last_error().decode() == "std::invalid_argument: " + str(e.value)
        assert lib.ju_set_source_size(a._h, SRC_W, SRC_H, 1) == 1 and b"filter" in lib.ju_last_error()
        assert a.get_source_size() == (SRC_W, SRC_H)
        # an odd YUV source
        a.set_source_size(SRC_W + 1, SRC_H + 1)
        odd = [np.zeros((SRC_H + 1, SRC_W + 1), np.uint8), np.zeros((SRC_H // 2, SRC_W + 1), np.uint8)]
        fr = R.host_frame(R.FMT_NV12, odd, CS)
        refused(lambda: a.process_frame(fr, R.host_frame(R.FMT_BGRX, [out])), "even")
        a.set_source_size(SRC_W, SRC_H)
        # a graphics resource as the input
        tex = torch.zeros((SRC_H, SRC_W * 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        try:
            assert lib.ju_debug_fake_gl_texture(21, tex.data_ptr(), SRC_W * 4, SRC_W, SRC_H, 4) == 0
            img = R.gl_image(21, output=False)
            refused(lambda: a.process(img, R.host_image(out)), "graphics resources")
            refused(lambda: a.set_source_mask(img), "host or device")
            R.release_gl_image(img)
        finally:
            lib.ju_debug_fake_gl_texture(0, None, 0, 0, 0, 0)
        # a mask with a short stride
        refused(lambda: a.set_source_mask(R.JuImage(out.ctypes.data, R.LOC_CPU, 8, 4, 4)), "stride")
        assert a.stat("source_mask") == 0 and a.stat("source_stage_frames") == 1
        # nothing ran: the stream goes on as its twin's
        for f in clip[1:]:
            assert np.array_equal(a.process_image(f), b.process_image(S.scale(f, h, w)))
        assert same_state(a, b)
