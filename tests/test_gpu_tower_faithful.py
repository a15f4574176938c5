"""The engine's residual tower against its rounding-faithful restatement (tests/tower_faithful.py), fed the
engine's own tower input of the same frame: `gen_in` for the 16-bit resident tower (generator/conv_1 is its layer
0), `trunk_a` (conv_1's fp16 output) for the 8-bit one.  The bounds are tower_faithful.BOUNDS.

The 8-bit towers here are two blocks deep whatever the geometry's own test uses (fp8_depth): the e4m3 matrix
instruction does not return the correctly rounded sum (tools/probes/fp8_mfma_accumulation_probe.hip), each of its
errors that flips an e4m3 rounding is a 1/16 step of one operand, and over more blocks these flips spread until the
trunk no longer tracks any restatement element for element.  Two blocks cover both convolutions, both halo
exchanges (the e4m3 input of a block is exchanged once the block before it is done) and the fp16 stream store."""

import dataclasses

import numpy as np
import pytest

from gpu_common import record
from helpers import M, gen_in_to_reference, oracle_config, small_config
from joshupscale_amd import runtime as R
import tower_faithful as TF

pytestmark = pytest.mark.gpu

KIND = {R.DTYPE_BF16: TF.BF16, R.DTYPE_F16: TF.F16, R.DTYPE_FP8: "fp8"}
DTYPES = [R.DTYPE_BF16, R.DTYPE_F16, R.DTYPE_FP8]
LEAKY = dict(gen_activation="lrelu", gen_negative_slope=0.2)


def fp8_depth(cfg, dtype):
    return dataclasses.replace(cfg, gen_blocks=min(cfg.gen_blocks, 2)) if dtype == R.DTYPE_FP8 else cfg


def restate(cfg, wts, dtype, tower_in):
    h, w = cfg.frame_height, cfg.frame_width
    ocfg = oracle_config(cfg)
    leaky = cfg.gen_activation == "lrelu"
    if dtype == R.DTYPE_FP8:
        return TF.tower8(tower_in.reshape(h, w, 64), wts, cfg.gen_blocks, ocfg.bn_eps, leaky, ocfg.gen_negative_slope)
    return TF.tower16(gen_in_to_reference(tower_in, h, w), wts, cfg.gen_blocks, ocfg.bn_eps, KIND[dtype], leaky,
                      ocfg.gen_negative_slope)


def check(what, cfg, wts, dtype, trunk, tower_in):
    st = TF.compare(trunk.reshape(cfg.frame_height, cfg.frame_width, 64), restate(cfg, wts, dtype, tower_in),
                    TF.F16 if dtype == R.DTYPE_FP8 else KIND[dtype])
    record(("tower-faithful",) + tuple(what) + (cfg.gen_blocks,), dtype, st)
    assert TF.within(st, KIND[dtype], cfg.gen_blocks), (what, st, TF.bounds(KIND[dtype], cfg.gen_blocks))
    return st


def run_case(what, cfg, wts, dtype, frames, monkeypatch):
    """Every frame: the engine's tower input and trunk against the restatement.  16-bit ReLU towers run under
    JU_TAIL=fused: the product kernel carries the tail in its last layer and writes no trunk."""
    if dtype != R.DTYPE_FP8:
        monkeypatch.setenv("JU_TAIL", "fused")
    rt = R.Runtime(M.serialize(cfg, wts), 0, dtype)
    try:
        what = tuple(what) + ("resident" if rt.stat("resident_tower") else "per-block",)
        for t, f in enumerate(frames):
            rt.process_image(f)
            tower_in = rt.read_tensor("trunk_a" if dtype == R.DTYPE_FP8 else "gen_in")
            check(tuple(what) + (t,), cfg, wts, dtype, rt.read_tensor("trunk"), tower_in)
    finally:
        rt.close()
        monkeypatch.delenv("JU_TAIL", raising=False)


SMALL = [(30, 48, 3), (34, 50, 2), (64, 96, 5), (40, 70, 24), (3, 131, 2), (130, 2, 2), (5, 7, 3), (4, 1030, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: R.DTYPE_NAMES[d])
@pytest.mark.parametrize("h,w,blocks", SMALL)
def test_tower_is_faithful_on_small_and_ragged_frames(h, w, blocks, dtype, monkeypatch):
    """The geometries of test_fp8_tower_matches_its_oracle: one round of tiles, ragged edges, the full depth,
    strips below one tile; three recurrent frames, so the tower's input differs from frame to frame."""
    cfg = fp8_depth(small_config(frame_height=h, frame_width=w, gen_blocks=blocks), dtype)
    run_case(("small", h, w), cfg, M.make_seeded_weights(cfg), dtype,
             M.synthetic_frames(3, h, w, seed=5, kind="smooth"), monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: R.DTYPE_NAMES[d])
@pytest.mark.parametrize("h,w,blocks", [(34, 50, 3), (40, 70, 24)])
def test_tower_is_faithful_for_a_leaky_generator(h, w, blocks, dtype, monkeypatch):
    """LeakyReLU: f32 activation before the store, e4m3 clamped on both sides."""
    cfg = fp8_depth(small_config(frame_height=h, frame_width=w, gen_blocks=blocks, **LEAKY), dtype)
    run_case(("lrelu", h, w), cfg, M.make_seeded_weights(cfg), dtype,
             M.synthetic_frames(3, h, w, seed=5, kind="smooth"), monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: R.DTYPE_NAMES[d])
@pytest.mark.parametrize("h,w", [(16, 8192), (4096, 32), (9, 8161), (512, 256), (129, 889)])
def test_tower_is_faithful_at_the_edges_of_the_resident_geometry(h, w, dtype, monkeypatch):
    """The shapes of test_resident_tower_at_the_edges_of_its_geometry (its model: 4 blocks, weights seed 11)."""
    cfg = fp8_depth(M.ModelConfig(frame_height=h, frame_width=w, gen_blocks=4), dtype)
    run_case(("resident-edge", h, w), cfg, M.make_seeded_weights(cfg, seed=11), dtype,
             M.synthetic_frames(2, h, w, seed=5, kind="smooth"), monkeypatch)


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=lambda d: R.DTYPE_NAMES[d])
def test_tower_is_faithful_with_more_tiles_than_workgroups(dtype, monkeypatch):
    """test_fp8_tower_multi_round_tiles' 328 x 416: more regions than the resident tower takes, so the per-block
    kernels run.  (Not the 8-bit engine: it has no resident form at this size, and its per-block forms update
    trunk_a in place -- there is no copy of its input to read.  Its per-block kernels are compared below on a
    geometry with a resident twin.)"""
    cfg = small_config(frame_height=328, frame_width=416, gen_blocks=1)
    run_case(("multi-round", 328, 416), cfg, M.make_seeded_weights(cfg), dtype,
             M.synthetic_frames(2, 328, 416, seed=11, kind="smooth"), monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: R.DTYPE_NAMES[d])
def test_tower_is_faithful_at_the_benchmark_size(dtype, monkeypatch):
    """psp-quality, 480 x 270: the benchmark's tower (49 convolutions on 16 bits; 8 bits: its first two blocks)."""
    cfg = fp8_depth(M.PRESETS["psp-quality"], dtype)
    run_case(("psp-quality",), cfg, M.make_seeded_weights(cfg), dtype,
             M.synthetic_frames(2, cfg.frame_height, cfg.frame_width, seed=5, kind="smooth"), monkeypatch)


@pytest.mark.parametrize("amax", [1.5, 0.2])
def test_fp8_tower_is_faithful_with_a_calibration_tensor(amax, monkeypatch):
    """generator/fp8_amax: a calibrated range (1.5) and the saturating one of
    test_fp8_calibration_tensor_and_saturation (0.2: everything above 0.4375 clips at 448 / 2^e)."""
    cfg = small_config(gen_blocks=2)
    wts = M.make_seeded_weights(cfg)
    wts["generator/fp8_amax"] = np.full(2 * cfg.gen_blocks, amax, np.float32)
    run_case(("fp8-amax", amax), cfg, wts, R.DTYPE_FP8, M.synthetic_frames(2, 30, 48, seed=5, kind="smooth"),
             monkeypatch)


@pytest.mark.parametrize("leaky", [False, True], ids=["relu", "lrelu"])
def test_fp8_block_and_per_conv_towers_are_faithful(leaky, monkeypatch):
    """JU_TOWER=layers / convs update trunk_a in place, so their input is taken from a resident twin runtime of the
    same model on the same frames (generator/conv_1 is the same launch in all three forms)."""
    cfg = small_config(frame_height=34, frame_width=70, gen_blocks=2, **(LEAKY if leaky else {}))
    wts = M.make_seeded_weights(cfg)
    blob = M.serialize(cfg, wts)
    frames = M.synthetic_frames(3, 34, 70, seed=1234, kind="noise")
    twin = R.Runtime(blob, 0, R.DTYPE_FP8)
    try:
        assert twin.stat("resident_tower") == 1
        inputs = []
        for f in frames:
            twin.process_image(f)
            inputs.append(twin.read_tensor("trunk_a").copy())
    finally:
        twin.close()
    for mode in ("layers", "convs"):
        monkeypatch.setenv("JU_TOWER", mode)
        rt = R.Runtime(blob, 0, R.DTYPE_FP8)
        try:
            assert rt.stat("resident_tower") == 0
            for t, f in enumerate(frames):
                rt.process_image(f)
                check(("fp8-" + mode, leaky, t), cfg, wts, R.DTYPE_FP8, rt.read_tensor("trunk"), inputs[t])
        finally:
            rt.close()
    monkeypatch.delenv("JU_TOWER")


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=lambda d: R.DTYPE_NAMES[d])
@pytest.mark.parametrize("preset", ["psp-quality", "small"])
def test_separate_tail_launch_gives_the_default_frames(preset, dtype, monkeypatch):
    """The trunk of a 16-bit ReLU tower is read under JU_TAIL=fused (tail as a launch of its own); engine.cpp states
    that launch is bit-identical to the tail carried in the tower's last layer: the frames and state are equal."""
    cfg = M.PRESETS["psp-quality"] if preset != "small" else small_config(frame_height=46, frame_width=70, gen_blocks=3)
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    frames = M.synthetic_frames(3, cfg.frame_height, cfg.frame_width, seed=11, kind="noise")
    runs = {}
    for mode in (None, "fused"):
        if mode:
            monkeypatch.setenv("JU_TAIL", mode)
        rt = R.Runtime(blob, 0, dtype)
        try:
            runs[mode] = ([rt.process_image(f).copy() for f in frames], rt.read_tensor("state").copy())
        finally:
            rt.close()
    monkeypatch.delenv("JU_TAIL")
    assert np.array_equal(runs[None][1], runs["fused"][1])
    for a, b in zip(runs[None][0], runs["fused"][0]):
        assert np.array_equal(a, b)
