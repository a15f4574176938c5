"""NV12 / I420 frames in look-ahead passes (ju_process_frames; engine_passes.cpp "YUV frames in look-ahead passes") -- needs an
MI355X.

The contract is byte equality with ju_process_frame called frame by frame: the expected bytes of every test come from
a twin runtime driven that way (the path tests/test_gpu_yuv.py holds to the numpy definition), never from the new entry
point; the one exception is the decode kernel's own test, which is held to the numpy definition directly.  Every plane,
every guard byte around it, the recurrent state, and the counters that say which path the frames took."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import yuv_reference as Y
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_yuv import CSS, FMTS, GUARD, LAYOUTS, DevPlane, out_planes, planes_of, run_debug, torch_dev

pytestmark = pytest.mark.gpu

BGRX, I420, NV12 = Y.FMT_BGRX, Y.FMT_I420, Y.FMT_NV12


# ---- 1. the decode kernel of a pass alone --------------------------------------------------------------------------
def run_items(fmts, css, w, h, outs, srcs):
    lib = R.load_library(True)
    n = len(fmts)
    ptrs, strides = [], []
    for planes in srcs:
        ptrs += [p.ptr for p in planes] + [None] * (3 - len(planes))
        strides += [p.stride for p in planes] + [0] * (3 - len(planes))
    rc = lib.ju_debug_yuv_items(n, (C.c_int * n)(*fmts), (C.c_int * n)(*css), w, h,
                                (C.c_void_p * n)(*[o.ptr for o in outs]), (C.c_ssize_t * n)(*[o.stride for o in outs]),
                                (C.c_void_p * (3 * n))(*ptrs), (C.c_ssize_t * (3 * n))(*strides))
    assert rc == 0, lib.ju_last_error()


@pytest.mark.parametrize("count", [1, 3, 8])
@pytest.mark.parametrize("mix", ["i420", "nv12", "mixed"])
def test_items_kernel_equals_the_numpy_definition_and_the_single_frame_kernel(mix, count):
    """1, 3 and 8 items in one launch; one format or both in one call; the four colour spaces and the five plane
    layouts (dense, padded, bottom-up, odd offsets) across the items; 30 x 46 (a width that is no multiple of 16, odd
    chroma counts) and 100 x 18.  Every item equals numpy's decode and ju_debug_yuv's bytes; guards and inputs intact."""
    rng = np.random.default_rng(11 + count)
    names = sorted(LAYOUTS)
    for (h, w) in [(46, 30), (18, 100)]:
        for shift in range(2):
            fmts, css, outs, singles, srcs, data = [], [], [], [], [], []
            for i in range(count):
                fmt = {"i420": I420, "nv12": NV12, "mixed": FMTS[(i + shift) % 2]}[mix]
                lay = LAYOUTS[names[(i + shift * 2) % len(names)]]
                y, u, v = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
                fmts.append(fmt)
                css.append(CSS[(i + shift) % len(CSS)])
                data.append((y, u, v))
                srcs.append([DevPlane(p, **lay) for p in planes_of(fmt, y, u, v)])
                mk = lambda: DevPlane(np.zeros((h, w, 4), np.uint8), pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
                outs.append(mk())
                singles.append(mk())
            run_items(fmts, css, w, h, outs, srcs)
            for i in range(count):
                want = Y.decode(*data[i], css[i])
                outs[i].check(want)
                run_debug(0, fmts[i], css[i], w, h, singles[i], srcs[i])
                assert (outs[i].buf == singles[i].buf).all(), (mix, count, i)
                for p, d in zip(srcs[i], planes_of(fmts[i], *data[i])):
                    p.check(d)


def run_single(fmt, cs, w, h, out, planes):
    """The format's single-kernel hook, op 0: planes -> BGRX."""
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    if fmt >= R.FMT_BGR24:
        rc = lib.ju_debug_rgb(0, fmt, w, h, out.ptr, out.stride, ptrs, strides)
    else:
        hook = (lib.ju_debug_yuv if fmt in FMTS else lib.ju_debug_yuv10 if fmt in (R.FMT_P010, R.FMT_I010)
                else lib.ju_debug_yuv_sampled)
        rc = hook(0, fmt, cs, w, h, out.ptr, out.stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


# all 21 formats in three launches, each mixing 4:2:0, 4:2:2 / 4:4:4 and RGB items and both sample depths; then NV12 alone
ITEM_LAUNCHES = [
    (R.FMT_I420, R.FMT_YUY2, R.FMT_BGR24, R.FMT_P010, R.FMT_I444, R.FMT_RGBP10, R.FMT_P210, R.FMT_BGR96F),
    (R.FMT_NV12, R.FMT_UYVY, R.FMT_RGB24, R.FMT_I410, R.FMT_BGRX64, R.FMT_RGBPS, R.FMT_RGBP8, R.FMT_RGBX),
    (R.FMT_I010, R.FMT_I422, R.FMT_RGBP16, R.FMT_I210, R.FMT_RGBPH),
    (R.FMT_NV12,)]


def test_items_kernel_dispatches_every_format_to_its_single_frame_strip():
    """Every format of the table as an item: its BGRX bytes equal those of the format's own single-kernel hook on the same
    planes (which the format's own suite holds to its numpy definition), guards and inputs intact.  34 x 6: two whole
    strips and a two-pixel tail, three row pairs, one workgroup, the upper half of a 4:2:0 item's threads returning.
    276 x 32: 18 strips with a four-pixel tail -- 576 threads, three workgroups per per-row item, of which a 4:2:0 item
    fills two and leaves the third idle.  The last launch is 4:2:0 alone: strips x H / 2 threads.  Random bytes in every
    plane (so junk in the bits and lanes a format ignores, and every kind of float), the four colour spaces in turn for
    the YUV items, a value outside them for the RGB items, which do not read it."""
    import test_gpu_rgb as G                                    # (imports this module: not at the top)
    assert sorted(f for launch in ITEM_LAUNCHES[:3] for f in launch) == sorted(
        list(G.NEW) + list(G.YS.NEW) + [I420, NV12, R.FMT_P010, R.FMT_I010])
    rng = np.random.default_rng(2026)
    for (w, h) in [(34, 6), (276, 32)]:
        for n, launch in enumerate(ITEM_LAUNCHES):
            fmts, css, outs, singles, srcs, held = list(launch), [], [], [], [], []
            for i, fmt in enumerate(launch):
                blank = G.blank(fmt, h, w)
                lay = G.layout(G.LAYOUT_NAMES[(i + n) % len(G.LAYOUT_NAMES)], blank[0].dtype.itemsize)
                css.append(9 + i if fmt >= R.FMT_BGR24 else CSS[(i + n) % len(CSS)])
                held.append([rng.integers(0, 256, (p.shape[0], p[0].nbytes), dtype=np.uint8) for p in blank])
                srcs.append([DevPlane(p, **lay) for p in held[i]])
                mk = lambda: DevPlane(np.zeros((h, w, 4), np.uint8), pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
                outs.append(mk())
                singles.append(mk())
            run_items(fmts, css, w, h, outs, srcs)
            for i, fmt in enumerate(launch):
                run_single(fmt, css[i], w, h, singles[i], srcs[i])
                want = singles[i]._rows(singles[i].buf.cpu().numpy()).reshape(h, w, 4)
                assert want[..., 3].max() == 0 and want.any(), (fmt, w, h)
                singles[i].check(want)
                outs[i].check(want)
                for p, d in zip(srcs[i], held[i]):
                    p.check(d)


# ---- frames, buffers and the twin -----------------------------------------------------------------------------------
def source(frame_bgrx, fmt, cs):
    """The planes of one input frame of the clip in the given format."""
    return [frame_bgrx] if fmt == BGRX else planes_of(fmt, *Y.encode(frame_bgrx, cs))


class HostPlane:
    """A [rows][row_bytes] plane inside a host array filled with GUARD; layouts as DevPlane's."""

    def __init__(self, data, pad=0, offset=0, flip=False):
        self.rows, self.row_bytes = data.shape[0], data.shape[1] * (data.shape[2] if data.ndim == 3 else 1)
        self.pitch, self.lead, self.flip = self.row_bytes + pad, 64 + offset, flip
        self.host = np.full(self.lead + self.rows * self.pitch + 64, GUARD, np.uint8)
        self._rows(self.host)[...] = data.reshape(self.rows, self.row_bytes)

    def _rows(self, buf):
        body = buf[self.lead:self.lead + self.rows * self.pitch].reshape(self.rows, self.pitch)[:, :self.row_bytes]
        return body[::-1] if self.flip else body

    @property
    def ptr(self):
        base = self.host.ctypes.data + self.lead
        return base + (self.rows - 1) * self.pitch if self.flip else base

    @property
    def stride(self):
        return -self.pitch if self.flip else self.pitch

    def check(self, want):
        exp = np.full_like(self.host, GUARD)
        self._rows(exp)[...] = want.reshape(self.rows, self.row_bytes)
        bad = np.flatnonzero(self.host != exp)
        assert bad.size == 0, (bad[:8], self.host[bad[:8]], exp[bad[:8]])


HOST_LAYOUTS = {"plain": dict(pad=0, flip=False), "padded": dict(pad=24, flip=False), "bottom-up": dict(pad=8, flip=True)}


class Side:
    """One side of a frame call: its planes in host or device memory with guard bytes around them."""

    def __init__(self, fmt, cs, loc, layout, planes, offset=0):
        lay = dict(HOST_LAYOUTS[layout], offset=offset)
        if fmt == BGRX:
            lay["pad"] *= 4                                     # (device BGRX rows stay 8-byte aligned)
        cls = HostPlane if loc == "host" else DevPlane
        self.fmt, self.planes = fmt, [cls(p, **lay) for p in planes]
        h, w = planes[0].shape[:2]
        self.frame = R._frame(fmt, cs, R.LOC_CPU if loc == "host" else R.LOC_DEVICE, w, h,
                              [p.ptr for p in self.planes], [p.stride for p in self.planes])

    def check(self, want):
        for p, e in zip(self.planes, want):
            p.check(e)


@dataclasses.dataclass
class Spec:
    """A frame of a call: (format, colour space, location, layout) of its input and of its output."""
    fin: int
    cin: int
    lin: str = "host"
    layin: str = "plain"
    fout: int = NV12
    cout: int = Y.CS_BT709_LIMITED
    lout: str = "host"
    layout: str = "plain"
    in_offset: int = 0


def twin_bytes(blob, dtype, frames, specs):
    """What ju_process_frame, called frame by frame on plain host frames of each spec's formats, writes; + the state."""
    cfg, _ = M.deserialize(blob)
    h, w = cfg.frame_height, cfg.frame_width
    want = []
    with R.Runtime(blob, 0, dtype) as rt:
        for f, s in zip(frames, specs):
            pin = source(f, s.fin, s.cin)
            pout = out_planes(s.fout, 4 * h, 4 * w)
            rt.process_frame(R.host_frame(s.fin, pin, s.cin), R.host_frame(s.fout, pout, s.cout))
            want.append(pout)
        state = rt.read_tensor("state").copy() if rt.recurrent else None
    return want, state


def make_sides(frames, specs, h, w):
    ins = [Side(s.fin, s.cin, s.lin, s.layin, source(f, s.fin, s.cin), offset=s.in_offset) for f, s in zip(frames, specs)]
    outs = [Side(s.fout, s.cout, s.lout, s.layout, out_planes(s.fout, 4 * h, 4 * w)) for s in specs]
    if any(s.lin == "device" or s.lout == "device" for s in specs):
        torch_dev()[0].cuda.synchronize()
    return ins, outs


def run_calls(rt, ins, outs, want, lengths):
    """The frames through ju_process_frames in calls of the given lengths; every output checked after its call."""
    t = 0
    for k in lengths:
        rt.process_frames([x.frame for x in ins[t:t + k]], [x.frame for x in outs[t:t + k]])
        for i in range(t, t + k):
            outs[i].check(want[i])
            ins[i].check([p._rows(p.host) for p in ins[i].planes])      # (inputs and their guards untouched)
        t += k


# ---- 2. host YUV frames in passes -----------------------------------------------------------------------------------
def model_blob(name):
    cfg = small_config() if name == "small" else M.PRESETS[name]
    return cfg, M.serialize(cfg, M.make_seeded_weights(cfg))


@pytest.mark.parametrize("model,dtype", [("psp-fast", R.DTYPE_F16), ("small", R.DTYPE_BF16)], ids=["psp-fast-fp16", "small-bf16"])
@pytest.mark.parametrize("fmt", [NV12, I420], ids=["nv12", "i420"])
def test_host_yuv_passes_give_the_frame_by_frame_bytes(fmt, model, dtype):
    """18 host frames as passes of 8, 5, 2 and 3, NV12 -> NV12 and I420 -> I420, plain / padded / bottom-up planes in
    and out independently: every plane and the state equal the twin's; all 18 frames rode in passes; all-host passes
    of one shape share one graph whatever the caller's addresses."""
    cfg, blob = model_blob(model)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED if fmt == NV12 else Y.CS_BT601_FULL
    n = 18
    frames = M.synthetic_frames(n, h, w, seed=97, kind="smooth")
    base = [Spec(fmt, cs, fout=fmt, cout=cs) for _ in range(n)]
    want, want_state = twin_bytes(blob, dtype, frames, base)
    for lay_in, lay_out in (("plain", "plain"), ("bottom-up", "bottom-up"), ("padded", "bottom-up"), ("bottom-up", "padded")):
        specs = [dataclasses.replace(s, layin=lay_in, layout=lay_out) for s in base]
        ins, outs = make_sides(frames, specs, h, w)
        with R.Runtime(blob, 0, dtype) as rt:
            run_calls(rt, ins, outs, want, (8, 5, 2, 3))
            assert np.array_equal(rt.read_tensor("state"), want_state)
            assert rt.stat("lookahead_yuv_frames") == n and rt.stat("lookahead_frames") == n
            assert rt.stat("lookahead_host_frames") == n and rt.stat("fallbacks") == 0
            # 8, 5, 2, 3 again on fresh host arrays: one capture per pass shape at most, then replays only
            captures = rt.stat("graph_captures")
            ins2, outs2 = make_sides(frames, specs, h, w)
            rt.reset()
            run_calls(rt, ins2, outs2, want, (8, 5, 2, 3))
            assert rt.stat("graph_captures") <= captures + 4
            rt.reset()
            ins3, outs3 = make_sides(frames[:8], specs[:8], h, w)
            before, captured = rt.stat("graph_replays"), rt.stat("graph_captures")
            run_calls(rt, ins3, outs3, want, (8,))
            assert rt.stat("graph_replays") == before + 1 and rt.stat("graph_captures") == captured


# ---- 3. device planes, cross formats --------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(NV12, I420), (BGRX, NV12), (NV12, BGRX), (I420, NV12)],
                         ids=["nv12-i420", "bgrx-nv12", "nv12-bgrx", "i420-nv12"])
def test_device_planes_and_cross_formats(pair):
    """Device planes with guard bytes, read and written in place: plain, padded and bottom-up; the input and output
    formats differ.  Same planes and state as the twin's, every guard byte intact."""
    fin, fout = pair
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    n = 7
    frames = M.synthetic_frames(n, h, w, seed=31, kind="smooth")
    lays = ["plain", "padded", "bottom-up"]
    specs = [Spec(fin, CSS[t % 4], "device", lays[t % 3], fout, CSS[(t + 1) % 4], "device", lays[(t + 1) % 3]) for t in range(n)]
    want, want_state = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        run_calls(rt, ins, outs, want, (5, 2))
        assert np.array_equal(rt.read_tensor("state"), want_state)
        assert rt.stat("lookahead_yuv_frames") == n and rt.stat("lookahead_frames") == n
        assert rt.stat("lookahead_host_frames") == 0 and rt.stat("fallbacks") == 0
        # the same tuples of device planes again: captured at their second use, replayed at the third
        for _ in range(2):
            rt.reset()
            run_calls(rt, ins, outs, want, (5, 2))
        assert rt.stat("graph_captures") == 2 and rt.stat("graph_replays") >= 2


# ---- 4. one call of every kind of frame ------------------------------------------------------------------------------
def test_one_call_mixing_every_kind_of_frame():
    """Host YUV, device YUV, host BGRX, device BGRX, and in the middle (index 4) a device BGRX input off 4-byte
    alignment, which no pass can take: passes of 4 on either side of it, the frame on its own between them."""
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(9, h, w, seed=19, kind="smooth")
    kinds = [Spec(NV12, 2, "host", "padded", I420, 0, "host", "bottom-up"),
             Spec(I420, 1, "device", "bottom-up", NV12, 3, "device", "padded"),
             Spec(BGRX, 0, "host", "bottom-up", BGRX, 0, "host", "padded"),
             Spec(BGRX, 0, "device", "padded", BGRX, 0, "device", "plain")]
    odd = Spec(BGRX, 0, "device", "plain", BGRX, 0, "device", "plain", in_offset=2)
    specs = kinds + [odd] + kinds
    want, want_state = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    assert ins[4].frame.planes[0] % 4 == 2
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        run_calls(rt, ins, outs, want, (9,))
        assert np.array_equal(rt.read_tensor("state"), want_state)
        assert rt.stat("lookahead_frames") == 8 and rt.stat("lookahead_yuv_frames") == 4
        assert rt.stat("lookahead_host_frames") == 4 and rt.stat("fallbacks") == 0


# ---- 5. BGRX only = ju_process_batch -----------------------------------------------------------------------------
def test_a_call_of_bgrx_frames_is_process_batch():
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    n = 11
    frames = M.synthetic_frames(n, h, w, seed=43, kind="noise")
    specs = [Spec(BGRX, 0, "device" if t % 3 else "host", "plain", BGRX, 0, "host" if t % 4 == 1 else "device", "plain")
             for t in range(n)]
    ins, outs = make_sides(frames, specs, h, w)
    ins_b, outs_b = make_sides(frames, specs, h, w)
    image = lambda s: R.JuImage(s.frame.planes[0], s.frame.location, s.frame.strides[0], s.frame.width, s.frame.height)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt, R.Runtime(blob, 0, R.DTYPE_BF16) as twin:
        twin.process_batch([image(s) for s in ins_b], [image(s) for s in outs_b])
        rt.process_frames([s.frame for s in ins], [s.frame for s in outs])
        for a, b in zip(outs, outs_b):
            got = [p.buf.cpu().numpy() if isinstance(p, DevPlane) else p.host for p in b.planes]
            a.check([p._rows(g) for p, g in zip(b.planes, got)])
        assert np.array_equal(rt.read_tensor("state"), twin.read_tensor("state"))
        for key in ("lookahead_frames", "lookahead_host_frames", "eager_runs", "graph_replays", "graph_captures"):
            assert rt.stat(key) == twin.stat(key), key
        assert rt.stat("lookahead_frames") == n and rt.stat("lookahead_yuv_frames") == 0


# ---- 6. other models --------------------------------------------------------------------------------------------------
def test_psp_quality_fp8_at_full_size():
    cfg, blob = model_blob("psp-quality")
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(5, h, w, seed=9, kind="smooth")
    specs = [Spec(NV12, 2, "host" if t % 2 else "device", "plain", NV12, 2, "host" if t % 2 else "device", "plain")
             for t in range(5)]
    want, want_state = twin_bytes(blob, R.DTYPE_FP8, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_FP8) as rt:
        run_calls(rt, ins, outs, want, (5,))
        assert np.array_equal(rt.read_tensor("state"), want_state)
        assert rt.stat("lookahead_yuv_frames") == 5 and rt.stat("fallbacks") == 0


@pytest.mark.parametrize("variant", ["flow-free", "temporal", "generic-flow", "brightness", "flow-resnet"])
def test_other_models_take_yuv_frames_in_one_call(variant, monkeypatch):
    """A flow-free model and the temporal output filter ride in passes; models without the batched flow plan take the
    same call frame by frame.  Same bytes in every case."""
    cfg = small_config()
    wts = None
    if variant == "flow-free":
        cfg, wts = flow_free(small_config())
    elif variant == "temporal":
        cfg = dataclasses.replace(M.PRESETS["psp-fast"], temporal_strength=0.6, temporal_window=3)
    elif variant == "generic-flow":
        monkeypatch.setenv("JU_FLOW_CONV", "generic")
    elif variant == "brightness":
        cfg = small_config(normalize_brightness=True)
    else:
        cfg = dataclasses.replace(M.PRESETS["psp-quality-flowres"], frame_height=64, frame_width=96)
    blob = M.serialize(cfg, wts if wts is not None else M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    n = 6
    frames = M.synthetic_frames(n, h, w, seed=3, kind="smooth")
    specs = [Spec(NV12 if t % 2 else I420, 2, "host" if t < 3 else "device", "plain", NV12, 2, "host" if t < 3 else "device",
                  "bottom-up") for t in range(n)]
    want, want_state = twin_bytes(blob, R.DTYPE_F16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt:
        run_calls(rt, ins, outs, want, (n,))
        if rt.recurrent:
            assert np.array_equal(rt.read_tensor("state"), want_state)
        in_passes = variant in ("flow-free", "temporal")
        assert rt.stat("lookahead_yuv_frames") == (n if in_passes else 0), variant
        assert rt.stat("lookahead_frames") == (n if in_passes else 0), variant


# ---- 7. overlapping planes --------------------------------------------------------------------------------------------
def test_an_output_plane_over_an_earlier_input_plane_starts_a_new_pass():
    """Frame 1's output Y plane lies over frame 0's input Y plane (device memory): frame 0 on its own, frames 1-2 as a
    pass.  And frame 2's input chroma plane inside frame 1's output chroma plane: it must be read after that write, so
    it starts a new pass too.  Same bytes as frame by frame on the same buffers."""
    torch, dev = torch_dev()
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    frames = M.synthetic_frames(4, h, w, seed=61, kind="smooth")
    src = [source(f, NV12, cs) for f in frames]

    def run(call):
        # arena: frame 0's input Y at its start, frame 1's output Y over all of it
        arena = torch.zeros(16 * h * w, dtype=torch.uint8, device=dev)
        arena[: h * w] = torch.from_numpy(src[0][0].reshape(-1)).to(dev)
        d_in = [[torch.from_numpy(p).to(dev) for p in s] for s in src]
        d_out = [[torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in out_planes(NV12, 4 * h, 4 * w)] for _ in frames]
        ins = [R.device_frame(NV12, w, h, [arena, d_in[0][1]], colorspace=cs)] + \
              [R.device_frame(NV12, w, h, d_in[t], colorspace=cs) for t in (1, 2, 3)]
        outs = [R.device_frame(NV12, 4 * w, 4 * h, d_out[0], colorspace=cs),
                R.device_frame(NV12, 4 * w, 4 * h, [arena, d_out[1][1]], colorspace=cs)] + \
               [R.device_frame(NV12, 4 * w, 4 * h, d_out[t], colorspace=cs) for t in (2, 3)]
        torch.cuda.synchronize()
        with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
            call(rt, ins, outs)
            stats = (rt.stat("lookahead_frames"), rt.stat("lookahead_yuv_frames"))
            state = rt.read_tensor("state").copy()
        got = [arena.cpu().numpy()] + [p.cpu().numpy() for planes in d_out for p in planes]
        return got, state, stats

    def one_by_one(rt, ins, outs):
        for a, b in zip(ins, outs):
            rt.process_frame(a, b)

    want, want_state, _ = run(one_by_one)
    got, state, stats = run(lambda rt, ins, outs: rt.process_frames(ins, outs))
    assert all(np.array_equal(g, e) for g, e in zip(got, want)) and np.array_equal(state, want_state)
    assert stats == (3, 3)                                      # frame 0 alone, frames 1-3 one pass

    # an input read out of an earlier frame's output: frame 2's UV plane is rows of frame 1's output UV plane
    def run2(call):
        d_in = [[torch.from_numpy(p).to(dev) for p in s] for s in src]
        d_out = [[torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in out_planes(NV12, 4 * h, 4 * w)] for _ in frames]
        ins = [R.device_frame(NV12, w, h, d_in[t], colorspace=cs) for t in range(4)]
        ins[2] = R.device_frame(NV12, w, h, [d_in[2][0], d_out[1][1]], [w, 4 * w], colorspace=cs)
        outs = [R.device_frame(NV12, 4 * w, 4 * h, d_out[t], colorspace=cs) for t in range(4)]
        torch.cuda.synchronize()
        with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
            call(rt, ins, outs)
            stats = rt.stat("lookahead_frames")
            state = rt.read_tensor("state").copy()
        return [p.cpu().numpy() for planes in d_out for p in planes], state, stats

    want, want_state, _ = run2(one_by_one)
    got, state, stats = run2(lambda rt, ins, outs: rt.process_frames(ins, outs))
    assert all(np.array_equal(g, e) for g, e in zip(got, want)) and np.array_equal(state, want_state)
    assert stats == 4                                           # passes of frames 0-1 and 2-3


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_a_refused_frame_refuses_the_call_and_leaves_the_runtime_unchanged():
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    frames = M.synthetic_frames(8, h, w, seed=2, kind="smooth")
    specs = [Spec(NV12, cs, fout=NV12, cout=cs) for _ in range(8)]
    want, want_state = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)

    def bad(frame, **kw):
        f = R.JuFrame()
        C.memmove(C.addressof(f), C.addressof(frame), C.sizeof(f))
        for k, val in kw.items():
            if k == "plane":
                f.planes[val] = None
            elif k == "stride":
                f.strides[0] = val
            else:
                setattr(f, k, val)
        return f

    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        run_calls(rt, ins, outs, want, (4,))
        state = rt.read_tensor("state").copy()
        idx = rt.stat("graph_replays"), rt.stat("eager_runs"), rt.stat("lookahead_frames")
        cases = {"odd height": (bad(ins[6].frame, height=h - 1), outs[6].frame, "even"),
                 "NULL plane": (bad(ins[6].frame, plane=1), outs[6].frame, "NULL"),
                 "wrong size": (bad(ins[6].frame, width=w + 2), outs[6].frame, "exactly"),
                 "short stride": (bad(ins[6].frame, stride=w - 2), outs[6].frame, "stride"),
                 "bad output": (ins[6].frame, bad(outs[6].frame, plane=0), "NULL"),
                 "unknown format": (bad(ins[6].frame, format=7), outs[6].frame, "format")}
        for name, (fi, fo, words) in cases.items():
            call_in = [ins[4].frame, ins[5].frame, fi, ins[7].frame]
            call_out = [outs[4].frame, outs[5].frame, fo, outs[7].frame]
            with pytest.raises(R.JoshUpscaleError) as e:
                rt.process_frames(call_in, call_out)
            assert e.value.code == 1 and "frame 2" in e.value.message and words in e.value.message, (name, e.value.message)
            assert "JU_" not in e.value.message
            assert np.array_equal(rt.read_tensor("state"), state), name
            assert (rt.stat("graph_replays"), rt.stat("eager_runs"), rt.stat("lookahead_frames")) == idx, name
        for o in outs[4:]:
            o.check(out_planes(NV12, 4 * h, 4 * w))             # (nothing was written)
        # the stream goes on as one that never saw the refused calls
        rt.process_frames([x.frame for x in ins[4:]], [x.frame for x in outs[4:]])
        for i in range(4, 8):
            outs[i].check(want[i])
        assert np.array_equal(rt.read_tensor("state"), want_state)


# ---- 9. the re-run's bookkeeping ---------------------------------------------------------------------------------------
def test_a_pass_that_is_run_again_gives_the_frame_by_frame_bytes():
    """ju_debug_set("pass_rerun", 1): a pass that completed is run again frame by frame -- the binding set and the
    counters restored -- as after a resident-tower report, but no kernel misbehaves and nothing falls back."""
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(12, h, w, seed=7, kind="smooth")
    specs = [Spec(NV12, 2, "host", "bottom-up", NV12, 2, "host", "padded") for _ in range(5)] + \
            [Spec(BGRX, 0, "device", "plain", BGRX, 0, "device", "padded") for _ in range(4)] + \
            [Spec(I420, 1, "device", "padded", NV12, 3, "host", "plain") for _ in range(3)]
    want, want_state = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        assert lib.ju_debug_set(b"pass_rerun", 1) == 0
        try:
            run_calls(rt, ins, outs, want, (5, 4))
        finally:
            lib.ju_debug_set(b"pass_rerun", 0)
        assert rt.stat("lookahead_frames") == 0 and rt.stat("lookahead_yuv_frames") == 0
        assert rt.stat("lookahead_host_frames") == 0 and rt.stat("fallbacks") == 0
        run_calls(rt, ins[9:], outs[9:], want[9:], (3,))        # switch off: the next pass counts
        assert rt.stat("lookahead_frames") == 3 and rt.stat("lookahead_yuv_frames") == 3
        assert np.array_equal(rt.read_tensor("state"), want_state)


# ---- 10. mixed with the other calls -----------------------------------------------------------------------------------
def test_process_frame_process_batch_and_process_frames_mix_on_one_runtime():
    cfg, blob = model_blob("small")
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(12, h, w, seed=13, kind="smooth")
    yuv = Spec(I420, 0, "host", "plain", NV12, 2, "device", "plain")
    rgb = Spec(BGRX, 0, "host", "plain", BGRX, 0, "host", "plain")
    specs = [yuv] * 3 + [yuv] + [rgb] * 3 + [yuv] * 4 + [rgb]
    want, want_state = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    image = lambda s: R.JuImage(s.frame.planes[0], s.frame.location, s.frame.strides[0], s.frame.width, s.frame.height)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        rt.process_frames([x.frame for x in ins[0:3]], [x.frame for x in outs[0:3]])
        rt.process_frame(ins[3].frame, outs[3].frame)
        rt.process_batch([image(x) for x in ins[4:7]], [image(x) for x in outs[4:7]])
        rt.process_frames([x.frame for x in ins[7:11]], [x.frame for x in outs[7:11]])
        rt.process(image(ins[11]), image(outs[11]))
        for o, e in zip(outs, want):
            o.check(e)
        assert np.array_equal(rt.read_tensor("state"), want_state)
        assert rt.stat("lookahead_frames") == 10 and rt.stat("lookahead_yuv_frames") == 7
