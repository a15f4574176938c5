"""Flow-free single-image models on the GPU (flow_arch "none", the reference's scripts/inference/onnx/remove_flow.py):
parity with the oracles of the recurrent twin R(F) (tests/flowfree_common.py), byte equality with R(F) on the GPU,
statelessness, every entry point, and that no flow work is done."""
import os
import subprocess

import numpy as np
import pytest

from flowfree_common import flow_free, recurrent_twin
from gpu_common import check_u8
from helpers import M, O, ROOT, oracle_config, psnr_u8, small_config
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

DTYPES = [R.DTYPE_BF16, R.DTYPE_F16, R.DTYPE_FP8]
DT_IDS = ["bf16", "fp16", "fp8"]


def fp8_allowed(cfg):
    return cfg.gen_filters == 64 and cfg.gen_blocks >= 1          # engine.cpp: the 8-bit tower's domain


def oracle_frame(frame, wts_r, ocfg):
    """The float64 oracle of R(F) on one frame with a zero history: F(frame) in real arithmetic."""
    h, w = ocfg.frame_height, ocfg.frame_width
    img = O.preprocess(O.bgrx_to_bgr(frame))
    raw = O.generator(img, np.zeros((4 * h, 4 * w, 3)), {k: np.asarray(v, np.float64) for k, v in wts_r.items()}, ocfg)
    return O.bgr_to_bgrx(O.postprocess(raw))


PARITY = {"small": small_config(), "w64": small_config(frame_width=64), "f32": small_config(gen_filters=32),
          "f128": small_config(gen_filters=128), "lrelu": small_config(gen_activation="lrelu", gen_negative_slope=0.2)}
# (fp8 only where the engine allows it)
PARITY_CASES = [pytest.param(cfg, dt, id=f"{name}-{dn}") for name, cfg in PARITY.items()
                for dt, dn in zip(DTYPES, DT_IDS) if dt != R.DTYPE_FP8 or fp8_allowed(cfg)]


@pytest.mark.parametrize("cfg,dtype", PARITY_CASES)
def test_parity_with_the_oracle_of_the_recurrent_twin(cfg, dtype):
    cfg_f, wts_f = flow_free(cfg)
    cfg_r, wts_r = recurrent_twin(cfg_f, wts_f)
    ocfg = oracle_config(cfg_r, fp8_tower=dtype == R.DTYPE_FP8)
    frames = M.synthetic_frames(3, cfg.frame_height, cfg.frame_width, seed=11, kind="smooth")
    with R.Runtime(M.serialize(cfg_f, wts_f), 0, dtype) as rt:
        assert not rt.recurrent
        for t in (2, 0, 1):                                   # any order: there is no history
            out = rt.process_image(frames[t])
            ref = oracle_frame(frames[t], wts_r, ocfg)
            if dtype == R.DTYPE_FP8:                          # against the oracle's restatement of the 8-bit scheme
                assert (out[..., 3] == 0).all() and psnr_u8(out, ref) >= 55.0, (t, psnr_u8(out, ref))
            else:
                check_u8(out, ref, dtype, ("flowfree", cfg.gen_filters, cfg.frame_width, cfg.gen_activation, t))


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "fp16"])
def test_full_size_preset_against_the_c_restatement_of_its_twin(dtype):
    """psp-quality-noflow at 480x270, whole frames, host and device paths, against the C restatement of R(F)
    (the C oracle reads recurrent containers only) on the benchmark's noise clip."""
    import torch
    from oracle.c_binding import CSession
    cfg = M.PRESETS["psp-quality-noflow"]
    wts = M.make_seeded_weights(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(2, h, w, seed=1234, kind="noise")
    cs = CSession(M.serialize(*recurrent_twin(cfg, wts)), h, w)
    refs = [cs.run(f).copy() for f in frames]
    cs.close()
    with R.Runtime(M.serialize(cfg, wts), 0, dtype) as rt:
        assert rt.stat("resident_tower") == 1
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(frames).to(dev)
        d_out = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for t, f in enumerate(frames):
            check_u8(rt.process_image(f), refs[t], dtype, ("noflow-full-host", t), clip="noise")
            rt.process(rt.device_image(d_in[t].data_ptr(), w, h), rt.device_image(d_out.data_ptr(), 4 * w, 4 * h))
            check_u8(d_out.cpu().numpy(), refs[t], dtype, ("noflow-full-device", t), clip="noise")


def twin_runtimes(cfg, dtype):
    cfg_f, wts_f = flow_free(cfg)
    return (R.Runtime(M.serialize(cfg_f, wts_f), 0, dtype),
            R.Runtime(M.serialize(*recurrent_twin(cfg_f, wts_f)), 0, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cfg", [small_config(), M.PRESETS["psp-quality"]], ids=["small", "full"])
def test_bytes_equal_the_recurrent_twin(cfg, dtype):
    """Same tower, same packed weights, a generator input that differs only in slots whose weights are zero: F's bytes
    are R(F)'s for every frame of a clip, on the host and the device path.  A difference is a staging or packing bug.
    ("full": F = remove_flow(psp-quality) = psp-quality-noflow at 480x270.)"""
    import torch
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(4, h, w, seed=5, kind="smooth")
    rf, rr = twin_runtimes(cfg, dtype)
    assert not rf.recurrent and rr.recurrent
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = [torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for t, f in enumerate(frames):
        a, b = rf.process_image(f), rr.process_image(f)
        assert np.array_equal(a, b), ("host", t, int(np.abs(a.astype(int) - b).max()))
    rr.reset()
    for t in range(len(frames)):
        for rt, o in zip((rf, rr), d_out):
            rt.process(rt.device_image(d_in[t].data_ptr(), w, h), rt.device_image(o.data_ptr(), 4 * w, 4 * h))
        assert torch.equal(d_out[0], d_out[1]), ("device", t)
    rf.close()
    rr.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_frames_are_independent(dtype):
    """No state: forwards, backwards, with ju_reset between frames, two runtimes interleaved and the brightness
    flag on or off all give the same per-frame bytes."""
    cfg = small_config()
    cfg_f, wts_f = flow_free(cfg)
    blob = M.serialize(cfg_f, wts_f)
    frames = M.synthetic_frames(5, cfg.frame_height, cfg.frame_width, seed=3, kind="smooth")
    rt = R.Runtime(blob, 0, dtype)
    fwd = [rt.process_image(f).copy() for f in frames]
    assert not np.array_equal(fwd[0], fwd[1])
    bwd = [rt.process_image(f).copy() for f in frames[::-1]][::-1]
    rst = []
    for f in frames:
        rst.append(rt.process_image(f).copy())
        rt.reset()
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(fwd, bwd, rst))
    rt2 = R.Runtime(blob, 0, dtype)
    for t in (4, 0, 3, 1, 2):
        assert np.array_equal(rt.process_image(frames[t]), fwd[t])
        assert np.array_equal(rt2.process_image(frames[(t + 2) % 5]), fwd[(t + 2) % 5])
    rt2.close()
    import dataclasses
    with R.Runtime(M.serialize(dataclasses.replace(cfg_f, normalize_brightness=True), wts_f), 0, dtype) as rb:
        assert all(np.array_equal(rb.process_image(f), o) for f, o in zip(frames, fwd))
    rt.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_every_entry_point_gives_the_bytes_of_ju_process(dtype, tmp_path):
    import torch
    cfg = small_config()
    cfg_f, wts_f = flow_free(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    n = 8
    frames = M.synthetic_frames(n, h, w, seed=21, kind="noise")
    rt = R.Runtime(M.serialize(cfg_f, wts_f), 0, dtype)
    base = [rt.process_image(f).copy() for f in frames]
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros((n, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ins = [rt.device_image(d_in[k].data_ptr(), w, h) for k in range(n)]
    outs = [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(n)]

    def device_outputs_match(what):
        got = d_out.cpu().numpy()
        for k in range(n):
            assert np.array_equal(got[k], base[k]), (what, k)
        d_out.zero_()
        torch.cuda.synchronize()

    # ju_process_batch in passes of 1, 3 and 8 (device and host frames)
    for la in (1, 3, 8):
        rt.set_lookahead(la)
        before = rt.stat("lookahead_frames")
        rt.process_batch(ins, outs)
        device_outputs_match(("batch", la))
        assert (rt.stat("lookahead_frames") > before) == (la > 1), la
        host_out = [np.zeros((4 * h, 4 * w, 4), np.uint8) for _ in range(n)]
        rt.process_batch([R.host_image(f) for f in frames], [R.host_image(o) for o in host_out])
        assert all(np.array_equal(a, b) for a, b in zip(host_out, base)), ("host batch", la)
    # ju_prepare_batch, then the pass replays its graphs
    assert rt.prepare_batch(ins[:4], outs[:4]) == 2
    captures = rt.stat("graph_captures")
    for _ in range(2):
        rt.process_batch(ins[:4], outs[:4])
        got = d_out.cpu().numpy()
        assert all(np.array_equal(got[k], base[k]) for k in range(4))
    assert rt.stat("graph_captures") == captures
    d_out.zero_()
    torch.cuda.synchronize()
    # ju_enqueue / ju_synchronize
    for k in range(n):
        rt.enqueue(ins[k], outs[k])
    rt.synchronize()
    device_outputs_match("enqueue")
    # ju_prepare_frames: a registered pair replays from its first frame
    d_pair = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    pair_out = rt.device_image(d_pair.data_ptr(), 4 * w, 4 * h)
    assert rt.prepare_frames(ins[1], pair_out) == 2
    captures, replays = rt.stat("graph_captures"), rt.stat("graph_replays")
    rt.process(ins[1], pair_out)
    assert np.array_equal(d_pair.cpu().numpy(), base[1])
    assert rt.stat("graph_captures") == captures and rt.stat("graph_replays") == replays + 1
    # host frames with negative strides (bottom-up in and out)
    for k in range(2):
        up = np.ascontiguousarray(frames[k][::-1])
        out = np.zeros((4 * h, 4 * w, 4), np.uint8)[::-1]
        rt.process_image(up[::-1], out=out)
        assert np.array_equal(out, base[k])
    # device frames at odd byte alignment and pitch
    off_in, pad_in, off_out, pad_out = 1, 3, 3, 5
    sin, sout = w * 4 + pad_in, 4 * w * 4 + pad_out
    for k in range(2):
        buf = np.zeros(off_in + h * sin + 16, np.uint8)
        for y in range(h):
            buf[off_in + y * sin:off_in + y * sin + w * 4] = frames[k][y].reshape(-1)
        bi = torch.from_numpy(buf).to(dev)
        bo = torch.full((off_out + 4 * h * sout + 16,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rt.process(rt.device_image(bi.data_ptr() + off_in, w, h, stride=sin),
                   rt.device_image(bo.data_ptr() + off_out, 4 * w, 4 * h, stride=sout))
        o = bo.cpu().numpy()
        rows = o[off_out:off_out + 4 * h * sout].reshape(4 * h, sout)
        assert np.array_equal(rows[:, :4 * w * 4].reshape(4 * h, 4 * w, 4), base[k])
        assert (o[:off_out] == 0xAB).all() and (rows[:-1, 4 * w * 4:] == 0xAB).all()
    rt.close()
    # the C++ plugin surface (tools/plugin_harness.cpp: the AviSynth and OBS call patterns)
    exe = os.path.join(ROOT, "build", "plugin_harness")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", ROOT, "harness"])
    cfg_h = M.ModelConfig(**{**cfg_f.__dict__, "compute_dtype": {R.DTYPE_BF16: M.DTYPE_BF16, R.DTYPE_F16: M.DTYPE_F16,
                                                                  R.DTYPE_FP8: M.DTYPE_FP8}[dtype]})
    model = str(tmp_path / "m.jupw")
    M.save(model, cfg_h, wts_f)
    frames[:5].tofile(str(tmp_path / "frames.raw"))
    r = subprocess.run([exe, model, str(tmp_path / "frames.raw"), "5", str(tmp_path / "out.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(str(tmp_path / "out.raw"), np.uint8).reshape(2, 4 * h, 4 * w, 4)
    assert np.array_equal(got[0], base[4]) and np.array_equal(got[1], base[4])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_no_flow_work(dtype):
    cfg = small_config()
    rf, rr = twin_runtimes(cfg, dtype)
    assert rf.stat("recurrent") == 0 and rr.stat("recurrent") == 1
    assert rf.time_steps("flow", 0)[1] == 0 and rf.time_steps("warp", 0)[1] == 0
    assert rf.time_steps("pack", 0)[1] == 0 and rf.time_steps("lr_pack", 0)[1] == 1
    assert rr.time_steps("flow", 0)[1] > 0 and rr.time_steps("warp", 0)[1] == 1
    assert rr.time_steps("lr_pack", 0)[1] == 0
    # the program: staging + the generator (no flow launches, no warp)
    assert rf.stat("launches_per_frame") < rr.stat("launches_per_frame")
    for name in ("flow", "state", "flow_in"):
        with pytest.raises(R.JoshUpscaleError):
            rf.read_tensor(name)
    rf.process_image(M.synthetic_frames(1, cfg.frame_height, cfg.frame_width, seed=2)[0])
    ms, n, _ = rf.time_steps("lr_pack", 20)
    assert n == 1 and ms > 0
    rf.close()
    rr.close()
