"""The output_flow model variant on the GPU (output "pre_warp", the reference's scripts/inference/onnx/output_flow.py):
every frame is the warped previous frame, byte for byte the post-process of the engine's own generator input; the
recurrent state is the plain model's; every entry point, every tower form."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import yuv_reference as Y
from gpu_common import TOL, check_u8, record
from helpers import M, O, ROOT, oracle_config, psnr_u8, small_config, u8_stats
from joshupscale_amd import runtime as R
from output_flow_common import frame_of_gen_in, oracle_frames
from test_gpu_parity import CASES, WIDTH_CASES

pytestmark = pytest.mark.gpu

DTYPES = [R.DTYPE_BF16, R.DTYPE_F16, R.DTYPE_FP8]
DT_IDS = ["bf16", "fp16", "fp8"]

CONFIGS = {
    "autoencoder": small_config(),
    "resnet": small_config(flow_arch="resnet", flow_pad_factor=0, flow_res_blocks=2),
    "lrelu": small_config(flow_activation="lrelu", gen_activation="lrelu", gen_negative_slope=0.2),
    "brightness": small_config(normalize_brightness=True),
    "temporal": small_config(temporal_strength=0.25),
    "temporal-window3": small_config(temporal_strength=0.25, temporal_window=3),
    "ragged": small_config(frame_height=35, frame_width=49),
}


def variant(cfg, seed=42):
    """(weights, plain container, variant container) of one model."""
    wts = M.make_seeded_weights(cfg, seed=seed)
    return wts, M.serialize(cfg, wts), M.serialize(*M.output_flow(cfg, wts))


def assert_exact(rt, out, what):
    """The definition: every B, G, R byte is the post-process (plus clamp) of the value the generator reads, X is 0."""
    want = frame_of_gen_in(rt.read_tensor("gen_in"), rt.input_height, rt.input_width)
    assert out.shape == want.shape
    assert (out[..., 3] == 0).all(), what
    assert np.array_equal(out, want), (what, int(np.abs(out.astype(int) - want).max()), float(np.mean(out != want)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_frames_are_the_post_process_of_the_generator_input(name, dtype):
    cfg = CONFIGS[name]
    _, _, blob_v = variant(cfg)
    frames = M.synthetic_frames(4, cfg.frame_height, cfg.frame_width, seed=5, kind="smooth")
    with R.Runtime(blob_v, 0, dtype) as rt:
        assert rt.output == "pre_warp"
        outs = []
        for t, f in enumerate(frames):
            outs.append(rt.process_image(f).copy())
            assert_exact(rt, outs[-1], (name, t))
        if not cfg.normalize_brightness:
            assert (outs[0][..., :3] == 127).all()               # the warp of a zero state
        assert not np.array_equal(outs[1], outs[0]) and not np.array_equal(outs[2], outs[1])


def still_cut_still(mode):
    """A temporal-filter model whose hard gate decides the same way in 16-bit arithmetic as in the oracle's, made as
    test_gpu_parity.py::test_temporal_filter_modes makes it: a still / cut / still clip and the threshold in the widest
    gap of the gate statistics the oracle sees."""
    a = M.synthetic_frames(1, 30, 48, seed=21, kind="smooth")
    b = M.synthetic_frames(1, 30, 48, seed=22, kind="noise")
    frames = np.concatenate([a, a, a, b, b, b])
    base = dict(temporal_strength=0.25, **mode)
    wts = M.make_seeded_weights(small_config(**base))
    probe = O.Session(wts, oracle_config(small_config(temporal_threshold=1.0, **base)))   # never cuts
    stats = []
    for f in frames:
        tr = {}
        probe.run(f, trace=tr)
        stats.append(np.asarray(tr["temporal_mean"], np.float64).ravel())
    allm = np.sort(np.concatenate(stats))
    lo, hi = int(0.2 * len(allm)), max(int(0.8 * len(allm)), int(0.2 * len(allm)) + 2)
    k = lo + int(np.argmax(allm[lo + 1:hi] - allm[lo:hi - 1]))
    thr = float(np.float32(0.5 * (allm[k] + allm[k + 1])))
    assert 0.0 < thr < 1.0 and allm[k + 1] - allm[k] > 0.02 * thr, "no clear gap for a hard gate"
    return small_config(temporal_threshold=thr, **base), frames


STATE_CASES = ["autoencoder", "resnet", "brightness", "ragged", "temporal-gap", "temporal-window16-gap", "temporal-window3"]


# (the thresholds of the -gap cases sit in a gap of the float64 statistics that is wide for 16-bit arithmetic, not for the
# 8-bit tower's deviation: 16-bit types only, as in test_gpu_parity.py)
STATE_PARAMS = [pytest.param(name, dt, id=f"{name}-{dn}") for name in STATE_CASES for dt, dn in zip(DTYPES, DT_IDS)
                if not (name.endswith("-gap") and dt == R.DTYPE_FP8)]


@pytest.mark.parametrize("name,dtype", STATE_PARAMS)
def test_state_and_history_are_the_plain_models(name, dtype):
    """A twin runtime from the plain container sees the same frames: recurrent state and LR history are bit-equal
    after every frame (with the temporal filter on: the filtered state), and the twin's frames are what they were
    (the oracle's, within the suite's bounds).  "temporal-window3" (a hard gate per 3-pixel window on a moving clip)
    has no threshold that every window is clear of, so 16-bit arithmetic and the oracle decide some windows
    differently -- in the plain model too; the suite compares no such model with the oracle, and neither does this
    case: it holds the state and the history only."""
    if name.endswith("-gap"):
        cfg, frames = still_cut_still(dict(temporal_window=16) if "window16" in name else {})
    else:
        cfg = CONFIGS[name]
        frames = M.synthetic_frames(4, cfg.frame_height, cfg.frame_width, seed=5, kind="smooth")
    wts, blob, blob_v = variant(cfg)
    fp8 = dtype == R.DTYPE_FP8
    sess = O.Session(wts, oracle_config(cfg, fp8_tower=fp8))
    with R.Runtime(blob_v, 0, dtype) as rt, R.Runtime(blob, 0, dtype) as twin:
        assert twin.output == "frame"
        differs = False
        for t, f in enumerate(frames):
            out, plain = rt.process_image(f), twin.process_image(f)
            if name != "temporal-window3":
                ref = sess.run(f)
                if fp8:                                           # against the oracle's restatement of the 8-bit scheme
                    assert (plain[..., 3] == 0).all() and psnr_u8(plain, ref) >= 55.0, (t, psnr_u8(plain, ref))
                else:
                    check_u8(plain, ref, dtype, ("output-flow-twin", name, t))
            for tensor in ("state", "flow_in"):
                assert np.array_equal(rt.read_tensor(tensor), twin.read_tensor(tensor)), (name, t, tensor)
            differs |= not np.array_equal(out, plain)
        assert differs


def lsb_bound(dtype):
    """|dv| <= eps on the generator input (TOL[dtype]["raw"], which test_gpu_parity.py holds gen_in to on these clips)
    moves (v + 0.5) * 255 by at most 255 eps, so the truncated (and clamped: 1-Lipschitz) bytes differ by at most
    floor(255 eps) + 1: 1 LSB for fp16 (eps = 0.001), 2 LSB for bf16 (eps = 0.007)."""
    return int(np.floor(255.0 * TOL[dtype]["raw"])) + 1


def against_the_oracle(cfg, dtype, seed, what):
    wts, _, blob_v = variant(cfg)
    frames = M.synthetic_frames(4, cfg.frame_height, cfg.frame_width, seed=seed, kind="smooth")
    _, want, _ = oracle_frames(cfg, wts, frames)
    bound = lsb_bound(dtype)
    assert bound == {R.DTYPE_F16: 1, R.DTYPE_BF16: 2}[dtype]
    with R.Runtime(blob_v, 0, dtype) as rt:
        for t, f in enumerate(frames):
            out = rt.process_image(f)
            st = u8_stats(out, want[t])
            record(("output-flow",) + tuple(what) + (t,), dtype, st)     # PSNR and frac_gt1: recorded, not asserted
            print("output-flow", what, t, st)
            assert (out[..., 3] == 0).all()
            assert st["max"] <= bound, (what, t, st)


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("arch,pad,h,w,blocks,extra", CASES)
def test_small_models_against_the_oracles_pre_warp(arch, pad, h, w, blocks, extra, dtype):
    cfg = small_config(frame_height=h, frame_width=w, gen_blocks=blocks, flow_arch=arch, flow_pad_factor=pad,
                       flow_res_blocks=2, **extra)
    against_the_oracle(cfg, dtype, 5, ("small", arch, h, w, sorted(extra)))


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name,h,w,kw", WIDTH_CASES, ids=[c[0] for c in WIDTH_CASES])
def test_nondefault_widths_against_the_oracles_pre_warp(name, h, w, kw, dtype):
    kw = dict(kw)
    kw.setdefault("gen_blocks", 3)
    against_the_oracle(small_config(frame_height=h, frame_width=w, **kw), dtype, 7, ("widths", name, h, w))


# ---------------------------------------------------------------------------------------------------------------
# every path gives the bytes of ju_process on host frames
# ---------------------------------------------------------------------------------------------------------------
# (a model with normalize_brightness takes no look-ahead pass: its batch calls run frame by frame, with the same bytes)
PATH_CONFIGS = {"plain": small_config(), "temporal": small_config(temporal_strength=0.25),
                "brightness-temporal": small_config(normalize_brightness=True, temporal_strength=0.25)}


def twin_bytes(blob_v, dtype, frames):
    """The frames, the final state: a twin runtime driven by ju_process on host frames (each frame checked against the
    definition on the way)."""
    with R.Runtime(blob_v, 0, dtype) as twin:
        base = []
        for t, f in enumerate(frames):
            base.append(twin.process_image(f).copy())
            assert_exact(twin, base[-1], ("twin", t))
        return base, twin.read_tensor("state").copy()


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(PATH_CONFIGS))
def test_single_frame_paths_give_the_bytes_of_ju_process(name, dtype):
    import torch
    cfg = PATH_CONFIGS[name]
    _, _, blob_v = variant(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    n = 5
    frames = M.synthetic_frames(n, h, w, seed=21, kind="smooth")
    base, base_state = twin_bytes(blob_v, dtype, frames)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    torch.cuda.synchronize()
    lib = R.load_library()
    rt = R.Runtime(blob_v, 0, dtype)

    def done(what):
        assert np.array_equal(rt.read_tensor("state"), base_state), what
        rt.reset()

    # host frames: padded rows, bottom-up rows
    for t, f in enumerate(frames):
        pin = np.zeros((h, w + 3, 4), np.uint8)
        pin[:, :w] = f
        pout = np.full((4 * h, 4 * w + 5, 4), 0xAB, np.uint8)
        rt.process_image(pin[:, :w], out=pout[:, :4 * w])
        assert np.array_equal(pout[:, :4 * w], base[t]) and (pout[:, 4 * w:] == 0xAB).all(), ("padded", t)
    done("padded")
    for t, f in enumerate(frames):
        up = np.ascontiguousarray(f[::-1])
        out = np.zeros((4 * h, 4 * w, 4), np.uint8)[::-1]
        rt.process_image(up[::-1], out=out)
        assert np.array_equal(out, base[t]), ("bottom-up", t)
    done("bottom-up")

    # device frames written in place by the warp kernel: 16-byte aligned rows; rows that alternate between 16- and
    # 8-byte alignment (base and pitch multiples of 8 only); bottom-up; and off the kernels' alignment (staged)
    def device_run(what, off, pitch, flip):
        rows = 4 * h
        replays = rt.stat("graph_replays") + rt.stat("eager_runs")
        for t in range(n):
            bo = torch.full((off + rows * pitch + 32,), 0xAB, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            first = bo.data_ptr() + off + ((rows - 1) * pitch if flip else 0)
            rt.process(rt.device_image(d_in[t].data_ptr(), w, h),
                       rt.device_image(first, 4 * w, 4 * h, stride=-pitch if flip else pitch))
            o = bo.cpu().numpy()
            img = o[off:off + rows * pitch].reshape(rows, pitch)
            got = img[:, :16 * w].reshape(rows, 4 * w, 4)
            assert np.array_equal(got[::-1] if flip else got, base[t]), (what, t)
            assert (o[:off] == 0xAB).all() and (img[:, 16 * w:] == 0xAB).all() and (o[off + rows * pitch:] == 0xAB).all(), (what, t)
        assert rt.stat("graph_replays") + rt.stat("eager_runs") == replays + n
        done(what)

    assert d_in.data_ptr() % 256 == 0
    device_run("device-16", 0, 16 * w, False)
    device_run("device-8", 8, 16 * w + 8, False)
    device_run("device-bottom-up", 16, 16 * w + 24, True)
    device_run("device-misaligned", 3, 16 * w + 5, False)

    # ju_enqueue / ju_synchronize, then a prepared pair
    d_out = torch.zeros((n, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ins = [rt.device_image(d_in[k].data_ptr(), w, h) for k in range(n)]
    outs = [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(n)]
    for k in range(n):
        rt.enqueue(ins[k], outs[k])
    rt.synchronize()
    got = d_out.cpu().numpy()
    assert all(np.array_equal(got[k], base[k]) for k in range(n)), "enqueue"
    done("enqueue")
    d_pair = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    d_src = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    pair = (rt.device_image(d_src.data_ptr(), w, h), rt.device_image(d_pair.data_ptr(), 4 * w, 4 * h))
    assert rt.prepare_frames(*pair) > 0
    captures = rt.stat("graph_captures")
    for t in range(n):
        d_src.copy_(d_in[t])
        torch.cuda.synchronize()
        rt.process(*pair)
        assert np.array_equal(d_pair.cpu().numpy(), base[t]), ("prepared", t)
    assert rt.stat("graph_captures") == captures
    done("prepared")

    # graphics resources through the test double (texture -> staging -> engine -> staging -> texture)
    in_pitch, out_pitch = w * 4 + 64, 4 * w * 4 + 128
    tex_in = torch.zeros((h, in_pitch), dtype=torch.uint8, device=dev)
    tex_out = torch.full((4 * h, out_pitch), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    try:
        assert lib.ju_debug_fake_gl_texture(21, tex_in.data_ptr(), in_pitch, w, h, 4) == 0
        assert lib.ju_debug_fake_gl_texture(22, tex_out.data_ptr(), out_pitch, 4 * w, 4 * h, 4) == 0
        img_in, img_out = R.gl_image(21, output=False), R.gl_image(22, output=True)
        for t, f in enumerate(frames):
            tex_in[:, :w * 4] = torch.from_numpy(f.reshape(h, w * 4)).to(dev)
            torch.cuda.synchronize()
            rt.process(img_in, img_out)
            got = tex_out.cpu().numpy()
            assert np.array_equal(got[:, :16 * w].reshape(4 * h, 4 * w, 4), base[t]), ("gl", t)
            assert (got[:, 16 * w:] == 0xAB).all()
        R.release_gl_image(img_in)
        R.release_gl_image(img_out)
    finally:
        lib.ju_debug_fake_gl_texture(0, None, 0, 0, 0, 0)
    done("gl")
    rt.close()


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(PATH_CONFIGS))
def test_lookahead_passes_give_the_bytes_of_ju_process(name, dtype):
    import torch
    cfg = PATH_CONFIGS[name]
    _, _, blob_v = variant(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    n = 8
    frames = M.synthetic_frames(n, h, w, seed=23, kind="smooth")
    base, base_state = twin_bytes(blob_v, dtype, frames)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros((n, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with R.Runtime(blob_v, 0, dtype) as rt:
        rt.set_lookahead(8)
        passes = not cfg.normalize_brightness
        ins = [rt.device_image(d_in[k].data_ptr(), w, h) for k in range(n)]
        outs = [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(n)]

        def check_device(what):
            got = d_out.cpu().numpy()
            for k in range(n):
                assert np.array_equal(got[k], base[k]), (what, k)
            assert np.array_equal(rt.read_tensor("state"), base_state), what
            d_out.zero_()
            torch.cuda.synchronize()
            rt.reset()

        before = rt.stat("lookahead_frames")
        rt.process_batch(ins, outs)
        assert (rt.stat("lookahead_frames") > before) == passes
        check_device("device 8")
        rt.process_batch(ins[:3], outs[:3])
        rt.process_batch(ins[3:], outs[3:])
        assert (rt.stat("lookahead_frames") > before + 8) == passes
        check_device("device 3 + 5")
        for split in ((8,), (3, 5)):
            host_out = [np.zeros((4 * h, 4 * w, 4), np.uint8) for _ in range(n)]
            t = 0
            for k in split:
                rt.process_batch([R.host_image(f) for f in frames[t:t + k]], [R.host_image(o) for o in host_out[t:t + k]])
                t += k
            assert all(np.array_equal(a, b) for a, b in zip(host_out, base)), ("host", split)
            assert np.array_equal(rt.read_tensor("state"), base_state)
            rt.reset()
        assert (rt.stat("lookahead_host_frames") > 0) == passes
        # a prepared tuple replays its graphs
        assert (rt.prepare_batch(ins[:4], outs[:4]) > 0) == passes
        captures = rt.stat("graph_captures")
        for _ in range(2):
            rt.process_batch(ins[:4], outs[:4])
            got = d_out.cpu().numpy()
            assert all(np.array_equal(got[k], base[k]) for k in range(4)), "prepared tuple"
            rt.reset()
        assert rt.stat("graph_captures") == captures


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "fp16"])
def test_group_of_three_variant_runtimes(dtype):
    import torch
    cfg = small_config(temporal_strength=0.25)
    _, _, blob_v = variant(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    n = 4
    frames = M.synthetic_frames(n + 2, h, w, seed=29, kind="smooth")
    clips = [frames[k:k + n] for k in range(3)]                     # every member its own clip
    bases = [twin_bytes(blob_v, dtype, c) for c in clips]
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros((3, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rts = [R.Runtime(blob_v, 0, dtype) for _ in range(3)]
    try:
        for t in range(n):
            R.process_group(rts, [rt.device_image(d_in[k + t].data_ptr(), w, h) for k, rt in enumerate(rts)],
                            [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k, rt in enumerate(rts)])
            got = d_out.cpu().numpy()
            for k in range(3):
                assert np.array_equal(got[k], bases[k][0][t]), (k, t)
        assert all(rt.stat("group_frames") == n for rt in rts)
        for k, rt in enumerate(rts):
            assert np.array_equal(rt.read_tensor("state"), bases[k][1]), k
            rt.reset()
        # host frames in a group
        for t in range(n):
            host_out = [np.zeros((4 * h, 4 * w, 4), np.uint8) for _ in range(3)]
            R.process_group(rts, [R.host_image(clips[k][t]) for k in range(3)], [R.host_image(o) for o in host_out])
            for k in range(3):
                assert np.array_equal(host_out[k], bases[k][0][t]), ("host", k, t)
    finally:
        for rt in rts:
            rt.close()


def test_group_of_a_variant_and_a_plain_runtime_is_refused():
    import torch
    cfg = small_config()
    _, blob, blob_v = variant(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(2, h, w, seed=31, kind="smooth")
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = torch.full((2, 4 * h, 4 * w, 4), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with R.Runtime(blob_v, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        a.process_image(frames[0])
        b.process_image(frames[0])
        states = [rt.read_tensor("state").copy() for rt in (a, b)]
        for members in ((a, b), (b, a)):
            with pytest.raises(R.JoshUpscaleError) as e:
                R.process_group(members, [rt.device_image(d_in[1].data_ptr(), w, h) for rt in members],
                                [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k, rt in enumerate(members)])
            assert e.value.code == 1 and "does not match" in e.value.message
        # nothing ran
        assert (d_out.cpu().numpy() == 0xAB).all()
        assert all(rt.stat("group_frames") == 0 for rt in (a, b))
        assert all(np.array_equal(rt.read_tensor("state"), s) for rt, s in zip((a, b), states))


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "fp16"])
def test_yuv_outputs_encode_the_variants_frame(dtype):
    """ju_process_frame / ju_process_frames with an NV12 (and an I420) output: the planes are tests/yuv_reference.py's
    encode of the BGRX frame ju_process gives -- the staging frame the encoder reads is the one the warp step wrote."""
    import torch
    cfg = small_config(temporal_strength=0.25)
    _, _, blob_v = variant(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    n = 6
    frames = M.synthetic_frames(n, h, w, seed=37, kind="smooth")
    base, base_state = twin_bytes(blob_v, dtype, frames)
    cs = R.CS_BT709_LIMITED
    want = []
    for b in base:
        y, u, v = Y.encode(b, cs)
        want.append((y, u, v, Y.to_nv12(u, v)))

    def nv12_planes():
        return [np.zeros((4 * h, 4 * w), np.uint8), np.zeros((2 * h, 4 * w), np.uint8)]

    with R.Runtime(blob_v, 0, dtype) as rt:
        for t, f in enumerate(frames):                              # frame by frame, host planes
            p = nv12_planes()
            rt.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(R.FMT_NV12, p, cs))
            assert np.array_equal(p[0], want[t][0]) and np.array_equal(p[1], want[t][3]), ("nv12", t)
        assert np.array_equal(rt.read_tensor("state"), base_state)
        rt.reset()
        for t, f in enumerate(frames):                              # I420
            p = [np.zeros((4 * h, 4 * w), np.uint8), np.zeros((2 * h, 2 * w), np.uint8), np.zeros((2 * h, 2 * w), np.uint8)]
            rt.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(R.FMT_I420, p, cs))
            assert all(np.array_equal(p[k], want[t][k]) for k in range(3)), ("i420", t)
        rt.reset()
        # look-ahead passes: host planes, then device planes
        rt.set_lookahead(8)
        outs = [nv12_planes() for _ in range(n)]
        rt.process_frames([R.host_frame(R.FMT_BGRX, [f]) for f in frames], [R.host_frame(R.FMT_NV12, p, cs) for p in outs])
        assert rt.stat("lookahead_yuv_frames") > 0
        for t in range(n):
            assert np.array_equal(outs[t][0], want[t][0]) and np.array_equal(outs[t][1], want[t][3]), ("pass host", t)
        assert np.array_equal(rt.read_tensor("state"), base_state)
        rt.reset()
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(frames).to(dev)
        d_out = [[torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in nv12_planes()] for _ in range(n)]
        torch.cuda.synchronize()
        rt.process_frames([R.device_frame(R.FMT_BGRX, w, h, [d_in[t]]) for t in range(n)],
                          [R.device_frame(R.FMT_NV12, 4 * w, 4 * h, d_out[t], colorspace=cs) for t in range(n)])
        for t in range(n):
            assert np.array_equal(d_out[t][0].cpu().numpy(), want[t][0]), ("pass device y", t)
            assert np.array_equal(d_out[t][1].cpu().numpy(), want[t][3]), ("pass device uv", t)
        assert np.array_equal(rt.read_tensor("state"), base_state)


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_FP8], ids=["bf16", "fp8"])
def test_plugin_surface_gives_the_bytes_of_ju_process(dtype, tmp_path):
    """tools/plugin_harness.cpp (the AviSynth and OBS call patterns of the C++ surface) on a variant model file."""
    cfg = dataclasses.replace(small_config(), compute_dtype={R.DTYPE_BF16: M.DTYPE_BF16, R.DTYPE_FP8: M.DTYPE_FP8}[dtype])
    wts = M.make_seeded_weights(cfg)
    cfg_v, _ = M.output_flow(cfg, wts)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(5, h, w, seed=41, kind="smooth")
    base, _ = twin_bytes(M.serialize(cfg_v, wts), dtype, frames)
    # the harness's AviSynth pattern: 16 mirrored warm-up frames (-fn, held at the last), then the clip
    warm = [min(-fn, 4) if fn < 0 else fn for fn in range(-16, 5)]
    avisynth, _ = twin_bytes(M.serialize(cfg_v, wts), dtype, frames[warm])
    exe = os.path.join(ROOT, "build", "plugin_harness")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", ROOT, "harness"])
    model = str(tmp_path / "m.jupw")
    M.save(model, cfg_v, wts)
    frames.tofile(str(tmp_path / "frames.raw"))
    r = subprocess.run([exe, model, str(tmp_path / "frames.raw"), "5", str(tmp_path / "out.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(str(tmp_path / "out.raw"), np.uint8).reshape(2, 4 * h, 4 * w, 4)
    assert np.array_equal(got[0], avisynth[-1]) and np.array_equal(got[1], base[4])
    assert not np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------------------------------------------------
# full size, saturation, tower forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,dtype", [("psp-quality", R.DTYPE_BF16), ("psp-quality", R.DTYPE_FP8),
                                          ("ps2-quality", R.DTYPE_BF16)], ids=["psp-bf16", "psp-fp8", "ps2-bf16"])
def test_full_size_presets(preset, dtype):
    """480x270 (the resident tower with the fused tail writes the scratch frame) and 640x448 (per-block towers)."""
    import torch
    cfg = M.PRESETS[preset]
    _, blob, blob_v = variant(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(3, h, w, seed=5, kind="smooth")
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with R.Runtime(blob_v, 0, dtype) as rt, R.Runtime(blob, 0, dtype) as twin:
        assert rt.stat("resident_tower") == twin.stat("resident_tower") == (1 if preset == "psp-quality" else 0)
        assert rt.stat("launches_per_frame") == twin.stat("launches_per_frame")        # no launch more
        for t in range(3):
            rt.process(rt.device_image(d_in[t].data_ptr(), w, h), rt.device_image(d_out.data_ptr(), 4 * w, 4 * h))
            assert_exact(rt, d_out.cpu().numpy(), (preset, "device", t))
            twin.process_image(frames[t])
            assert np.array_equal(rt.read_tensor("state"), twin.read_tensor("state")), (preset, t)
        rt.reset()
        for t in range(2):
            assert_exact(rt, rt.process_image(frames[t]), (preset, "host", t))


def clip_a(h, w):
    f = M.synthetic_frames(4, h, w, seed=5, kind="smooth").copy()
    f[1::2, ..., :3] //= 4                                          # odd frames darkened to a quarter
    return f


def clip_b(h, w):
    a = np.zeros((h, w, 4), np.uint8)
    a[8:20, 10:30, :3] = 255                                        # black with a white patch
    b = np.full((h, w, 4), 255, np.uint8)                           # all white
    f = np.stack([a, b, a, b])
    f[..., 3] = 255
    return f


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("clip", ["a", "b"])
def test_out_of_range_pre_warp_saturates(clip, dtype):
    """normalize_brightness: pre_warp = warp(state) + b_t leaves +-0.5 when the brightness jumps between frames.  The
    bytes there are 0 / 255, not wrapped.  The oracle says where: x = (pre_warp + 0.5) * 255 >= 256 or < 0.  The
    engine's generator input is within eps = TOL[dtype]["raw"] of the oracle's, so its x is within m = 255 eps: where the
    oracle has x >= 256 + m the byte must be 255, where it has x < -m it must be 0 (fp16: m = 0.255, and 255 / 0 follow
    for EVERY out-of-range position, since 256 - m > 255 and m < 1; asserted so).  Everywhere the bytes stay within
    floor(255 eps) + 1 of the clipped expectation -- a wrapped byte would be some 250 off."""
    cfg = small_config(normalize_brightness=True)
    h, w = cfg.frame_height, cfg.frame_width
    assert (h, w) == (30, 48)
    frames = clip_a(h, w) if clip == "a" else clip_b(h, w)
    wts, _, blob_v = variant(cfg, seed=42)
    _, want, pre = oracle_frames(cfg, wts, frames)
    x = [(p + 0.5) * 255.0 for p in pre]
    # the oracle really leaves the range on this clip
    if clip == "a":
        assert all((x[t] < 0).sum() > 5000 for t in (1, 3)) and all((x[t] >= 256).sum() == 0 for t in range(4))
    else:
        assert all((x[t] >= 256).sum() > 10000 for t in (1, 3)) and (x[2] < 0).sum() > 1000
        assert max(p.max() for p in pre) > 1.3
    m = 255.0 * TOL[dtype]["raw"]
    bound = lsb_bound(dtype)
    with R.Runtime(blob_v, 0, dtype) as rt:
        for t, f in enumerate(frames):
            out = rt.process_image(f)
            assert_exact(rt, out, (clip, t))
            got = out[..., :3]
            st = u8_stats(out, want[t])
            print("saturation", clip, t, st, int((x[t] >= 256).sum()), int((x[t] < 0).sum()))
            hi, lo = x[t] >= 256 + m, x[t] < -m
            if t in (1, 3):
                assert (hi if clip == "b" else lo).sum() > 1000
            assert (got[hi] == 255).all() and (got[lo] == 0).all(), (clip, t)
            if dtype == R.DTYPE_F16:
                assert (got[x[t] >= 256] == 255).all() and (got[x[t] < 0] == 0).all(), (clip, t)
            assert st["max"] <= bound, (clip, t, st)


def test_output_select_stat_and_property():
    cfg = small_config(gen_blocks=1)
    _, blob, blob_v = variant(cfg)
    for hooks in (True, False):                                     # the test flavour and the product library
        with R.Runtime(blob, 0, hooks=hooks) as plain, R.Runtime(blob_v, 0, hooks=hooks) as rt:
            assert plain.stat("output_select") == 0 and plain.output == "frame"
            assert rt.stat("output_select") == 1 and rt.output == "pre_warp"
    # a flow-free model with the word set is refused at creation, with the loaders' message
    from flowfree_common import flow_free
    cfg_f, wts_f = flow_free(cfg)
    bad = M.serialize(dataclasses.replace(cfg_f, output="pre_warp"), wts_f, validate=False)
    with pytest.raises(R.JoshUpscaleError, match=M.NO_FLOW_PRE_WARP):
        R.Runtime(bad, 0)


def form_run(blob_v, blob, dtype, frames, what):
    with R.Runtime(blob_v, 0, dtype) as rt, R.Runtime(blob, 0, dtype) as twin:
        for t, f in enumerate(frames):
            assert_exact(rt, rt.process_image(f), (what, t))
            twin.process_image(f)
            assert np.array_equal(rt.read_tensor("state"), twin.read_tensor("state")), (what, t)
        return rt.stat("resident_tower"), rt.stat("launches_per_frame")


@pytest.mark.parametrize("name", ["relu", "lrelu", "gen32"])
def test_every_tower_form(name, monkeypatch):
    """Every u8 writer of the frame program gets the scratch frame: the resident tower with its fused tail, the
    diagnostic schedules of that kernel (their tail is a launch of its own), the separate fused tail, the two-kernel
    tail, per-block and per-layer towers (pipelined and plain block kernels), the 8-bit towers in every form."""
    cfg = {"relu": small_config(frame_height=34, frame_width=50), "gen32": small_config(gen_filters=32),
           "lrelu": small_config(gen_activation="lrelu", gen_negative_slope=0.2)}[name]
    _, blob, blob_v = variant(cfg)
    frames = M.synthetic_frames(3, cfg.frame_height, cfg.frame_width, seed=11, kind="smooth")
    lib = R.load_library()
    seen = set()
    for dtype in (R.DTYPE_BF16, R.DTYPE_F16):
        for tower in ("resident", "layers", "convs"):
            for tail in ("tower", "fused", "split"):
                monkeypatch.setenv("JU_TOWER", tower)
                monkeypatch.setenv("JU_TAIL", tail)
                seen.add(form_run(blob_v, blob, dtype, frames, (name, dtype, tower, tail)))
        monkeypatch.delenv("JU_TAIL")
        monkeypatch.setenv("JU_TOWER", "resident")
        try:                                                        # the plain and the general schedule of the resident kernel
            lib.ju_debug_set(b"tower_variant", 8)
            form_run(blob_v, blob, dtype, frames, (name, dtype, "variant 8"))
            lib.ju_debug_set(b"tower_variant", 0)
            lib.ju_debug_set(b"tower_fast", 0)
            form_run(blob_v, blob, dtype, frames, (name, dtype, "general"))
        finally:
            lib.ju_debug_set(b"tower_variant", 0)
            lib.ju_debug_set(b"tower_fast", 1)
        monkeypatch.setenv("JU_TOWER", "layers")
        try:
            lib.ju_debug_set(b"res_block_plain", 1)
            form_run(blob_v, blob, dtype, frames, (name, dtype, "plain block kernel"))
        finally:
            lib.ju_debug_set(b"res_block_plain", 0)
    if cfg.gen_filters == 64:                                       # (other widths: one program, the generic kernels and the two-kernel tail)
        assert len(seen) > 1                                        # the switches did select different programs
        # the 8-bit tower's domain
        try:
            for tower in ("resident", "layers", "convs"):
                monkeypatch.setenv("JU_TOWER", tower)
                for form in (0, 1, 2):
                    lib.ju_debug_set(b"fp8_block_form", form)
                    form_run(blob_v, blob, R.DTYPE_FP8, frames, (name, "fp8", tower, form))
        finally:
            lib.ju_debug_set(b"fp8_block_form", 0)
