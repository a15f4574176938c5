"""The rounding-faithful tower restatement (tests/tower_faithful.py) on the CPU: it is the oracle's tower when its
roundings are off, it stays within the quantisation noise when they are on, and the trunk comparison's bounds
(tower_faithful.BOUNDS, which test_gpu_tower_faithful.py holds the engine to) pass a restatement that only sums in
another order and fail restatements with one kernel-style bug in one convolution."""

import numpy as np
import pytest

from helpers import M, O, err, oracle_config, small_config
import tower_faithful as TF

H, W = 40, 70


def _traces(blocks, fp8, **kw):
    """Oracle traces of the second frame (recurrent state non-zero: the whole generator input is live)."""
    cfg = small_config(frame_height=H, frame_width=W, gen_blocks=blocks, **kw)
    wts = M.make_seeded_weights(cfg)
    ocfg = oracle_config(cfg, fp8_tower=fp8)
    sess = O.Session(wts, ocfg)
    frames = M.synthetic_frames(2, H, W, seed=5, kind="smooth")
    tr = {}
    sess.run(frames[0])
    sess.run(frames[1], tr)
    return cfg, wts, ocfg, tr


@pytest.mark.parametrize("leaky", [False, True], ids=["relu", "lrelu"])
def test_without_its_roundings_the_restatement_is_the_oracle(leaky):
    kw = dict(gen_activation="lrelu", gen_negative_slope=0.2) if leaky else {}
    cfg, wts, ocfg, tr = _traces(3, False, **kw)
    got = TF.tower16(tr["gen_in_ref"], wts, 3, ocfg.bn_eps, TF.BF16, leaky, ocfg.gen_negative_slope, rounding=False)
    assert err(got, tr["trunk"])["rel_to_max"] <= 1e-12
    cfg, wts, ocfg, tr = _traces(3, True, **kw)
    got = TF.tower8(tr["gen_head"], wts, 3, ocfg.bn_eps, leaky, ocfg.gen_negative_slope, rounding=False)
    assert err(got, tr["trunk"])["rel_to_max"] <= 1e-12


@pytest.mark.parametrize("leaky", [False, True], ids=["relu", "lrelu"])
def test_with_its_roundings_the_restatement_stays_within_the_noise(leaky):
    """16-bit: within a few units of the stream type's rounding of the float oracle's trunk.  8-bit: the criterion
    _fp8_case holds the engine to -- trunk RMS against the 8-bit oracle at most 0.95 x the quantisation noise (the
    8-bit oracle's distance to the float one)."""
    kw = dict(gen_activation="lrelu", gen_negative_slope=0.2) if leaky else {}
    cfg, wts, ocfg, tr = _traces(3, False, **kw)
    for dt, tol in ((TF.BF16, 2.0 ** -8 * 4), (TF.F16, 2.0 ** -11 * 4)):
        got = TF.tower16(TF.to_stream(tr["gen_in_ref"], dt), wts, 3, ocfg.bn_eps, dt, leaky, ocfg.gen_negative_slope)
        e = err(got, tr["trunk"])
        assert 0 < e["rel_to_max"] <= tol, (dt, e)
    tf = tr["trunk"]
    cfg, wts, ocfg, t8 = _traces(3, True, **kw)
    got = TF.tower8(TF.to_f16(t8["gen_head"]), wts, 3, ocfg.bn_eps, leaky, ocfg.gen_negative_slope)
    noise = err(t8["trunk"], tf)["rms"]
    assert 0 < err(got, t8["trunk"])["rms"] <= 0.95 * noise


def _tower(kind, blocks):
    cfg, wts, ocfg, tr = _traces(blocks, kind == "fp8")
    if kind == "fp8":
        x = TF.to_f16(tr["gen_head"])
        return 2 * blocks, lambda **k: TF.tower8(x, wts, blocks, ocfg.bn_eps, **k)
    x = TF.to_stream(tr["gen_in_ref"], kind)
    return 1 + 2 * blocks, lambda **k: TF.tower16(x, wts, blocks, ocfg.bn_eps, kind, **k)


# (kind, argument): rows 16 and columns 32 are region edges of both resident towers (32 x 16 regions, RH <= 16)
MUTANTS = [("halo_row", 16), ("halo_col", 32), ("last_row", None), ("k_slice", 0), ("tap", None), ("truncate", None)]


@pytest.mark.parametrize("kind,blocks", [(TF.BF16, 3), (TF.F16, 3), (TF.BF16, 24), (TF.F16, 24), ("fp8", 2)])
def test_the_bounds_pass_another_summation_order_and_fail_every_mutant(kind, blocks):
    """The restatement summed in float32 (BLAS order, taps reversed: a stand-in for the MFMA order) passes the
    bounds the GPU tests hold the engine to; each mutant fails them, in the first, a middle and the last
    convolution of the tower -- 3 and 24 blocks for the 16-bit towers, 2 for the 8-bit one (its bounds' depth)."""
    n, run = _tower(kind, blocks)
    stream = TF.F16 if kind == "fp8" else kind
    ref = run()
    st = TF.compare(run(accumulate="f32"), ref, stream)
    assert TF.within(st, kind, blocks), ("reordered", st, TF.bounds(kind, blocks))
    passed = []
    for layer in (0, n // 2, n - 1):
        for name, arg in MUTANTS:
            st = TF.compare(run(mutant=(name, layer, arg)), ref, stream)
            if TF.within(st, kind, blocks):
                passed.append((name, layer, st))
    assert not passed, passed


def test_the_store_roundings_are_the_kernels():
    """Round to nearest even from the fp32 value (pack4, floatToBF16), truncation only in the mutant."""
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20])
    assert TF.to_bf16(x).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7]
    assert TF.to_bf16(x, truncate=True).tolist() == [1.0, 1.0 + 2.0 ** -7, -1.0, 1.0]
    y = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.0, 2.0 ** -25 * 3])
    assert TF.to_f16(y).tolist() == [1.0, 1.0 + 2.0 ** -9, 65504.0, 2.0 ** -23]
    assert TF.to_f16(y, truncate=True).tolist() == [1.0, 1.0 + 2.0 ** -10, 65504.0, 2.0 ** -24]
    # e4m3 of the ReLU form clamps at 0 and 448; the LeakyReLU form on both sides
    assert TF.e4m3(np.array([-3.0, 500.0, 0.3]), 0, False).tolist() == [0.0, 448.0, 0.3125]
    assert TF.e4m3(np.array([-500.0, 0.3]), 1, True).tolist() == [-224.0, 0.3125]
    assert TF.ulp(np.array([1.0, 0.0]), TF.BF16).tolist() == [2.0 ** -7, 2.0 ** -133]


@pytest.mark.parametrize("blocks", [2, 24])
def test_the_8bit_tower_in_another_summation_order_agrees_to_a_unit(blocks):
    """e4m3 x e4m3 products are exact, so the float32-reordered 8-bit restatement differs from the float64 one only
    where an fp32 sum lands next to a rounding midpoint: measured, no element more than 1 unit off at 2 blocks and
    a few parts per million at 24 (frame 2 of this clip).  The 8-bit engine deviates more than this because its
    matrix instruction's sums are not correctly rounded (tower_faithful.BOUNDS)."""
    n, run = _tower("fp8", blocks)
    ref = run()
    st = TF.compare(run(accumulate="f32"), ref, TF.F16)
    assert st["frac_gt1ulp"] <= 2e-5 and st["max_ulp"] <= 6 and abs(st["mean_ulp"]) <= 1e-3, st
