"""8-bit 4:2:0 frame I/O on the GPU (ju_process_frame / ju_enqueue_frame, csrc/colour_kernels.hip): the conversion
kernels alone against the numpy definition (tests/yuv_reference.py), byte for byte; every frame call against a twin
runtime fed BGRX frames through ju_process and the numpy conversions; locations, strides, mixed calls, other models
and the refused calls."""

import ctypes as C

import numpy as np
import pytest

import yuv_reference as Y
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

GUARD = 0xA5
CSS = sorted(Y.COLORSPACE_NAMES)
FMTS = [Y.FMT_I420, Y.FMT_NV12]
FMT_IDS = ["i420", "nv12"]


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


# ---- device planes with guard bytes ------------------------------------------------------------------------------
class DevPlane:
    """A [rows][row_bytes] plane inside a device buffer filled with GUARD: rows `pad` bytes apart beyond row_bytes,
    the first row `offset` bytes past a 256-aligned start plus a 64-byte guard, bottom-up when `flip`."""

    def __init__(self, data, pad=0, offset=0, flip=False):
        torch, dev = torch_dev()
        self.rows, self.row_bytes = data.shape[0], data.shape[1] * (data.shape[2] if data.ndim == 3 else 1)
        self.pitch = self.row_bytes + pad
        self.lead = 64 + offset
        self.size = self.lead + self.rows * self.pitch + 64
        self.flip = flip
        self.host = np.full(self.size, GUARD, np.uint8)
        self._place(self.host, data)
        self.buf = torch.from_numpy(self.host.copy()).to(dev)

    def _rows(self, buf):
        body = buf[self.lead:self.lead + self.rows * self.pitch].reshape(self.rows, self.pitch)[:, :self.row_bytes]
        return body[::-1] if self.flip else body

    def _place(self, buf, data):
        self._rows(buf)[...] = data.reshape(self.rows, self.row_bytes)

    @property
    def ptr(self):
        base = self.buf.data_ptr() + self.lead
        return base + (self.rows - 1) * self.pitch if self.flip else base

    @property
    def stride(self):
        return -self.pitch if self.flip else self.pitch

    def check(self, want):
        """The plane equals `want` byte for byte and every other byte of the buffer is still GUARD."""
        got = self.buf.cpu().numpy()
        exp = self.host.copy()
        self._place(exp, want)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (bad[:8], got[bad[:8]], exp[bad[:8]])


def planes_of(fmt, y, u, v):
    return [y, u, v] if fmt == Y.FMT_I420 else [y, Y.to_nv12(u, v)]


def run_debug(direction, fmt, cs, w, h, bgrx: DevPlane, planes):
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    rc = lib.ju_debug_yuv(direction, fmt, cs, w, h, bgrx.ptr, bgrx.stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


def content(kind, h, w, rng):
    if kind == "random":
        return [rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    if kind == "zero":
        return [np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)]
    if kind == "full":
        return [np.full((h, w), 255, np.uint8)] + [np.full((h // 2, w // 2), 255, np.uint8)] * 2
    # extreme chroma: U, V at 0 / 255 in a checkerboard of cells, luma random
    cb = (np.indices((h // 2, w // 2)).sum(0) % 2 * 255).astype(np.uint8)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8), cb, 255 - cb]


# sizes: odd chroma counts (30 x 46 -> 15 x 23), a width that is not a multiple of 16, a 1080p-like strip
SIZES = [(46, 30), (2, 2), (30, 48), (18, 100), (64, 1920)]
LAYOUTS = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=32, offset=0, flip=False),
           "bottom-up": dict(pad=16, offset=0, flip=True), "odd-offset": dict(pad=3, offset=1, flip=False),
           "odd-flip": dict(pad=5, offset=3, flip=True)}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_conversion_kernels_equal_the_numpy_definition(fmt, layout):
    rng = np.random.default_rng(5)
    lay = LAYOUTS[layout]
    for (h, w) in SIZES:
        for cs in CSS:
            for kind in ("random", "zero", "full", "extreme"):
                y, u, v = content(kind, h, w, rng)
                # decode: planes -> BGRX
                src = [DevPlane(p, **lay) for p in planes_of(fmt, y, u, v)]
                out = DevPlane(np.zeros((h, w, 4), np.uint8), pad=lay["pad"] * 4, offset=lay["offset"],
                               flip=lay["flip"])
                run_debug(0, fmt, cs, w, h, out, src)
                out.check(Y.decode(y, u, v, cs))
                for p, d in zip(src, planes_of(fmt, y, u, v)):
                    p.check(d)                                  # (inputs untouched)
                # encode: BGRX (X random: ignored) -> planes
                bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if kind == "random" else Y.decode(y, u, v, cs)
                inb = DevPlane(bgrx, pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
                ey, eu, ev = Y.encode(bgrx, cs)
                dst = [DevPlane(np.zeros_like(p), **lay) for p in planes_of(fmt, ey, eu, ev)]
                run_debug(1, fmt, cs, w, h, inb, dst)
                for p, want in zip(dst, planes_of(fmt, ey, eu, ev)):
                    p.check(want)


# ---- end to end against a twin runtime ------------------------------------------------------------------------------
def yuv_clip(n, h, w, cs, seed=3):
    """Planes of the smooth clip (encode of its BGRX frames): realistic, moving content."""
    frames = M.synthetic_frames(n, h, w, seed=seed, kind="smooth")
    return [Y.encode(f, cs) for f in frames]


def host_in(fmt, yuv, cs):
    y, u, v = yuv
    planes = planes_of(fmt, y, u, v)
    return planes, R.host_frame(fmt, planes, cs)


def out_planes(fmt, h, w):
    if fmt == Y.FMT_BGRX:
        return [np.zeros((h, w, 4), np.uint8)]
    if fmt == Y.FMT_NV12:
        return [np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)]
    return [np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)]


def expect_out(fmt, bgrx, cs):
    if fmt == Y.FMT_BGRX:
        return [bgrx]
    y, u, v = Y.encode(bgrx, cs)
    return planes_of(fmt, y, u, v)


SMALL = [pytest.param(R.DTYPE_BF16, id="bf16"), pytest.param(R.DTYPE_F16, id="fp16"),
         pytest.param(R.DTYPE_FP8, id="fp8")]


@pytest.mark.parametrize("dtype", SMALL)
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_yuv_input_equals_process_of_the_decoded_frame(fmt, dtype):
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED if fmt == Y.FMT_NV12 else Y.CS_BT601_FULL
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        for yuv in yuv_clip(5, h, w, cs):
            _, fin = host_in(fmt, yuv, cs)
            got = out_planes(Y.FMT_BGRX, 4 * h, 4 * w)
            a.process_frame(fin, R.host_frame(R.FMT_BGRX, got))
            want = b.process_image(Y.decode(*yuv, cs))
            assert (got[0] == want).all()


@pytest.mark.parametrize("dtype", SMALL)
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_yuv_output_equals_the_encoded_output_of_process(fmt, dtype):
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_FULL if fmt == Y.FMT_NV12 else Y.CS_BT601_LIMITED
    frames = M.synthetic_frames(5, h, w, seed=8, kind="smooth")
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        for f in frames:
            got = out_planes(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got, cs))
            for g, e in zip(got, expect_out(fmt, b.process_image(f), cs)):
                assert (g == e).all()


def test_full_size_psp_quality_nv12_to_nv12():
    """psp-quality bf16 at 480 x 270: NV12 in, NV12 out, on host and device frames."""
    torch, dev = torch_dev()
    cfg = M.PRESETS["psp-quality"]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        for t, yuv in enumerate(yuv_clip(4, h, w, cs, seed=9)):
            want = expect_out(Y.FMT_NV12, b.process_image(Y.decode(*yuv, cs)), cs)
            if t % 2 == 0:
                _, fin = host_in(Y.FMT_NV12, yuv, cs)
                got = out_planes(Y.FMT_NV12, 4 * h, 4 * w)
                a.process_frame(fin, R.host_frame(R.FMT_NV12, got, cs))
            else:
                din = [torch.from_numpy(p).to(dev) for p in planes_of(Y.FMT_NV12, *yuv)]
                dout = [torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in out_planes(Y.FMT_NV12, 4 * h, 4 * w)]
                torch.cuda.synchronize()
                a.process_frame(R.device_frame(R.FMT_NV12, w, h, din, colorspace=cs),
                                R.device_frame(R.FMT_NV12, 4 * w, 4 * h, dout, colorspace=cs))
                got = [d.cpu().numpy() for d in dout]
            for g, e in zip(got, want):
                assert (g == e).all(), t


def dev_copy(arr, dev, flip):
    """A device copy of a host plane, described top-down or bottom-up: (tensor, pointer, stride)."""
    import torch
    data = np.ascontiguousarray(arr[::-1] if flip else arr)
    t = torch.from_numpy(data).to(dev)
    pitch = data.strides[0]
    ptr = t.data_ptr() + (data.shape[0] - 1) * pitch if flip else t.data_ptr()
    return t, ptr, (-pitch if flip else pitch)


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_locations_and_row_orders_give_the_same_bytes(fmt):
    """Host / device x top-down / bottom-up, on both sides: one runtime per variant, all equal to the first."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    clip = yuv_clip(3, h, w, cs, seed=4)
    results = {}
    for loc in ("host", "device"):
        for flip in (False, True):
            outs = []
            with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
                for yuv in clip:
                    pin = planes_of(fmt, *yuv)
                    pout = out_planes(fmt, 4 * h, 4 * w)
                    if loc == "host":
                        # bottom-up: the rows lie in reverse in memory and a [::-1] view addresses the first logical
                        # row (the last in memory) with a negative stride
                        vin = [np.ascontiguousarray(p[::-1])[::-1] if flip else p for p in pin]   # (kept alive)
                        fin = R.host_frame(fmt, vin, cs)
                        rt.process_frame(fin, R.host_frame(fmt, [p[::-1] for p in pout] if flip else pout, cs))
                        outs.append([p[::-1].copy() if flip else p.copy() for p in pout])
                    else:
                        ins = [dev_copy(p, dev, flip) for p in pin]
                        outs_d = [dev_copy(p, dev, flip) for p in pout]
                        torch.cuda.synchronize()
                        rt.process_frame(R.device_frame(fmt, w, h, [x[1] for x in ins], [x[2] for x in ins], cs),
                                         R.device_frame(fmt, 4 * w, 4 * h, [x[1] for x in outs_d],
                                                        [x[2] for x in outs_d], cs))
                        got = [x[0].cpu().numpy() for x in outs_d]
                        outs.append([g[::-1] if flip else g for g in got])
            results[(loc, flip)] = outs
    first = results[("host", False)]
    for key, outs in results.items():
        for t in range(len(clip)):
            for g, e in zip(outs[t], first[t]):
                assert (g == e).all(), (key, t)


def test_mixed_calls_on_one_runtime():
    """ju_process, ju_process_frame and ju_enqueue_frame + ju_synchronize on one stream equal all-BGRX ju_process
    calls on the twin composed with the numpy conversions."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT601_LIMITED
    clip = yuv_clip(6, h, w, cs, seed=12)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        for t, yuv in enumerate(clip):
            bgrx_in = Y.decode(*yuv, cs)
            ref = b.process_image(bgrx_in)
            mode = t % 3
            if mode == 0:                                       # plain ju_process on the decoded frame
                got = a.process_image(bgrx_in)
                assert (got == ref).all(), t
            elif mode == 1:                                     # I420 host in, NV12 host out
                _, fin = host_in(Y.FMT_I420, yuv, cs)
                pout = out_planes(Y.FMT_NV12, 4 * h, 4 * w)
                a.process_frame(fin, R.host_frame(R.FMT_NV12, pout, cs))
                for g, e in zip(pout, expect_out(Y.FMT_NV12, ref, cs)):
                    assert (g == e).all(), t
            else:                                               # NV12 device in, I420 device out, enqueued
                din = [torch.from_numpy(p).to(dev) for p in planes_of(Y.FMT_NV12, *yuv)]
                dout = [torch.zeros(p.shape, dtype=torch.uint8, device=dev)
                        for p in out_planes(Y.FMT_I420, 4 * h, 4 * w)]
                torch.cuda.synchronize()
                a.enqueue_frame(R.device_frame(R.FMT_NV12, w, h, din, colorspace=cs),
                                R.device_frame(R.FMT_I420, 4 * w, 4 * h, dout, colorspace=cs))
                a.synchronize()
                for g, e in zip([d.cpu().numpy() for d in dout], expect_out(Y.FMT_I420, ref, cs)):
                    assert (g == e).all(), t


@pytest.mark.parametrize("variant", ["flow-free", "temporal"])
def test_other_models_take_yuv_frames(variant):
    if variant == "flow-free":
        cfg, wts = flow_free(small_config())
    else:
        cfg = small_config(temporal_strength=0.25, temporal_threshold=0.5)
        wts = M.make_seeded_weights(cfg)
    blob = M.serialize(cfg, wts)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert a.recurrent == (variant != "flow-free")
        for yuv in yuv_clip(4, h, w, cs, seed=6):
            ref = b.process_image(Y.decode(*yuv, cs))
            y, u = a.process_yuv(yuv[0], Y.to_nv12(yuv[1], yuv[2]), None, R.FMT_NV12, cs)
            ey, euv = expect_out(Y.FMT_NV12, ref, cs)
            assert (y == ey).all() and (u == euv).all()


def test_refused_calls_leave_the_runtime_unchanged():
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    clip = yuv_clip(3, h, w, cs, seed=2)
    torch, dev = torch_dev()
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        good_in_planes, good_in = host_in(Y.FMT_NV12, clip[0], cs)
        pout = out_planes(Y.FMT_NV12, 4 * h, 4 * w)
        good_out = R.host_frame(R.FMT_NV12, pout, cs)

        def bad(**kw):
            f = R.JuFrame()
            C.memmove(C.addressof(f), C.addressof(good_in), C.sizeof(f))
            for k, val in kw.items():
                if k == "plane":
                    f.planes[val] = None
                elif k == "stride":
                    f.strides[0] = val
                else:
                    setattr(f, k, val)
            return f
        cases = {
            "odd width": (bad(width=w - 1), good_out, "even"),
            "wrong size": (bad(width=w + 2), good_out, "exactly"),
            "NULL plane": (bad(plane=1), good_out, "NULL"),
            "unknown format": (bad(format=7), good_out, "format"),
            "unknown colour space": (bad(colorspace=9), good_out, "colour space"),
            "graphics resource": (bad(location=R.LOC_GRAPHICS_RESOURCE), good_out, "graphics"),
            "short stride": (bad(stride=w - 2), good_out, "stride"),
            "bad output": (good_in, bad(height=h), "exactly"),
        }
        for name, (fi, fo, words) in cases.items():
            with pytest.raises(R.JoshUpscaleError) as e:
                a.process_frame(fi, fo)
            assert e.value.code == 1 and words in e.value.message, (name, e.value.message)
        # a host frame handed to ju_enqueue_frame
        with pytest.raises(R.JoshUpscaleError) as e:
            a.enqueue_frame(good_in, good_out)
        assert e.value.code == 1 and "device" in e.value.message
        # nothing ran: the stream goes on as its twin's
        for yuv in clip:
            got = a.process_yuv(yuv[0], yuv[1], yuv[2], R.FMT_I420, cs, out_format=R.FMT_BGRX)
            assert (got == b.process_image(Y.decode(*yuv, cs))).all()
        del good_in_planes


def test_bgrx_frames_behave_as_process():
    """A BGRX ju_frame pair is ju_process: host and the direct device path, same bytes as the twin."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(4, h, w, seed=1, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        d_out = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        for t, f in enumerate(frames):
            ref = b.process_image(f)
            if t % 2:
                d_in = torch.from_numpy(f).to(dev)
                torch.cuda.synchronize()
                a.process_frame(R.device_frame(R.FMT_BGRX, w, h, [d_in]),
                                R.device_frame(R.FMT_BGRX, 4 * w, 4 * h, [d_out]))
                got = d_out.cpu().numpy()
            else:
                got = np.zeros((4 * h, 4 * w, 4), np.uint8)
                a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(R.FMT_BGRX, [got]))
            assert (got == ref).all(), t
