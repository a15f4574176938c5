"""Every launch plan of the flow net's convolution kernels gives the default plan's bytes -- needs an MI355X.

flow_block_kernel (flow_kernels.hip), conv_splitk_kernel (splitk_kernels.hip) and conv_mfma_kernel (conv_kernels.hip)
each choose a launch plan -- tile height, cout blocks per workgroup, tile form, staging depth -- from the tensor's
size, the CU count and the number of look-ahead frames.  An output element's terms are added in the same order under
every plan (the launchers' comments say so; conv_mfma_kernel: chunks in order, taps and k-steps in order inside a
chunk, whatever nb / rw / the staging depth, conv_kernels.hip convChunkMfma and the two chunk loops of
conv_mfma_kernel), so the claim under test is EQUALITY: np.array_equal of the flow head, every per-layer flow
activation, the generator input, the recurrent state and the frame, against the default plan's run of the same model
and frames.  No tolerance is involved; the default plan itself is held to the float64 oracle at the two new shapes
(test_default_plan_matches_the_oracle), so equality with it means something.

At the shapes the rest of the suite runs, the cost rules pick the smallest plan almost everywhere; here a plan is
FORCED per runtime (JU_FLOW_TILE, JU_SPLITK_PLAN, JU_CONV_TILE, JU_CONV_DBUF, JU_RES_BLOCK: read where the runtime is
constructed) and ju_plan_report says what the launchers really launched: a forced value the shape does not have is
ignored by its launcher, and every case asserts from the report that its plan ran.  The (block shape, tile height)
pairs that exist are taken from the report's `heights` field, not restated here.

Shapes: the smallest at which every level of the flow net has at least two tiles in both directions with a partial
last one, for the tallest tile --
  ragged  100 x 268 (pads to 104 x 272): levels 104x272, 52x136, 26x68, 13x34; 10 / 5 / 3 / 2 tile columns of 30 whose
          last is 2 / 16 / 8 / 2 wide; at every height of every block two tile rows or more, the last partial; the
          split-K level has an odd height (13)
  exact   120 x 240 (no padding): levels 120x240, 60x120, 30x60, 15x30; the last tile column ends on the image edge at
          every level, the heights 20, 10 and 6 divide the rows they tile
  single  30 x 48: a forced tall tile is ONE partial tile
"""

import contextlib
import functools
import os

import numpy as np
import pytest

from gpu_common import TOL, check_u8
from helpers import M, O, err, gen_in_to_reference, oracle_config, small_config
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

SHAPES = {"ragged": (100, 268), "exact": (120, 240), "single": (30, 48)}
DTYPES = [R.DTYPE_F16, R.DTYPE_BF16]
# every switch that selects a path or a plan of the flow net: a case states all it wants, the rest is unset
SWITCHES = ("JU_FLOW_TILE", "JU_SPLITK_PLAN", "JU_CONV_TILE", "JU_CONV_DBUF", "JU_RES_BLOCK", "JU_UPSAMPLE", "JU_PACK",
            "JU_POOL", "JU_FLOW_WIDE", "JU_FLOW_CONV", "JU_TOWER", "JU_FLOW")
LRELU = (("flow_activation", "lrelu"),)
N_FRAMES = 3


def config(shape, extra=()):
    h, w = SHAPES[shape]
    return small_config(frame_height=h, frame_width=w, gen_blocks=1, **dict(extra))


@functools.lru_cache(maxsize=None)
def model(shape, extra=()):
    cfg = config(shape, extra)
    wts = M.make_seeded_weights(cfg)
    return cfg, wts, M.serialize(cfg, wts)


@functools.lru_cache(maxsize=None)
def clip(shape):
    h, w = SHAPES[shape]
    frames = M.synthetic_frames(N_FRAMES, h, w, seed=31, kind="smooth")
    frames.setflags(write=False)
    return frames


def tensor_names(cfg):
    """What ju_read_tensor names of the flow net and behind it: every per-layer activation, the head, the generator
    input, the recurrent state and the frame history."""
    names = []
    for k in range(1, 2 * (len(cfg.flow_filters) // 2) + 1):
        names += ["flow/block_%d/%s" % (k, t) for t in ("a_1", "a_2", "resample")]
    if len(cfg.flow_filters) % 2:
        names.append("flow/a_1")
    return names + ["flow", "flow_in", "gen_in", "state"]


@contextlib.contextmanager
def runtime(blob, dtype, env):
    """A runtime constructed under exactly the switches of `env`.  They are read by the constructor: the environment is
    put back BEFORE the runtime runs a frame, so a plan that were looked up per launch would show as the default's."""
    keep = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(dict(env))
        rt = R.Runtime(blob, 0, dtype)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        yield rt
    finally:
        rt.close()


def run_frames(rt, frames, names):
    got = []
    for f in frames:
        d = {"frame": rt.process_image(f).copy()}
        for n in names:
            d[n] = rt.read_tensor(n)
        got.append(d)
    return got


def default_run(shape, dtype, extra=(), env=()):
    """The default plan's run under the path switches `env`: per frame every tensor, and the plan report.  The run of
    the default model on the default path is computed once per (shape, dtype) and shared; nobody writes to it."""
    return _default_run_shared(shape, dtype) if not extra and not env else _default_run(shape, dtype, extra, env)


@functools.lru_cache(maxsize=None)
def _default_run_shared(shape, dtype):
    return _default_run(shape, dtype, (), ())


def _default_run(shape, dtype, extra, env):
    cfg, _, blob = model(shape, extra)
    with runtime(blob, dtype, env) as rt:
        got = run_frames(rt, clip(shape), tensor_names(cfg))
        report = rt.plan_report()
    for d in got:
        for a in d.values():
            a.setflags(write=False)
    return got, report


def assert_same(got, ref, what):
    assert len(got) == len(ref)
    for t, (a, b) in enumerate(zip(got, ref)):
        for n in b:
            assert np.array_equal(a[n], b[n]), (what, "frame %d" % t, n, float(np.abs(a[n].astype(np.float64) - b[n]).max()))


def block_key(p):
    return (p["cin"], p["cmid"], p["ups"], p["pool"], p["outk"], p["pack"], p["indep"])


def flow_blocks(report, items=1, outk=(0, 1)):
    return [p for p in report if p["kernel"] == "flow_block" and p["items"] == items and p["outk"] in outk]


def check_forced_tile(report, tile, items=1, outk=(0, 1)):
    """Every block shape that has the height ran it; returns the (block shape, height) pairs that ran it."""
    ran = set()
    for p in flow_blocks(report, items, outk):
        assert p["rows"] in p["heights"], p
        if tile in p["heights"]:
            assert p["rows"] == tile, ("the forced height did not run", tile, p)
            ran.add((block_key(p), tile))
    return ran


# the one-launch blocks of the default flow net (16(12) -> 32 -> 64 -> 128 | 256 -> 128 -> 64 -> 32): cin, cmid, ups, pool,
# outk, pack, indep -- the paths below differ in the instantiations they reach, and each case asserts its set
ENCODER = {(32, 64, 0, 1, 0, 0, 0), (64, 128, 0, 1, 0, 0, 0)}
FUSED = ENCODER | {(16, 32, 0, 1, 0, 1, 0), (256, 128, 1, 0, 0, 0, 0), (128, 64, 1, 0, 0, 0, 0), (64, 32, 1, 0, 1, 0, 0)}
PATHS = {
    "fused": ((), FUSED),
    # the decoder blocks and the head behind upsample2_kernel launches: their non-UPS instantiations
    "upsample-split": ((("JU_UPSAMPLE", "split"),),
                       ENCODER | {(16, 32, 0, 1, 0, 1, 0), (256, 128, 0, 0, 0, 0, 0), (128, 64, 0, 0, 0, 0, 0), (64, 32, 0, 0, 1, 0, 0)}),
    # the first block behind pack_frames_kernel: its instantiation without PACK
    "pack-split": ((("JU_PACK", "split"),), (FUSED - {(16, 32, 0, 1, 0, 1, 0)}) | {(16, 32, 0, 1, 0, 0, 0)}),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flow_block_tile_heights_give_the_default_bytes(shape, path, dtype):
    """Case 1: flow_block_kernel at every height the report lists for every block shape -- a separate instantiation
    with its own LDS layout each (FbGeom; the 256 -> 128 decoder block at 4 and 6 rows: XPAIR, two input planes resident
    at a time) -- on the fused path, behind separate upsampling launches and behind a separate packing launch."""
    env, blocks = PATHS[path]
    cfg, _, blob = model(shape)
    ref, report = default_run(shape, dtype, (), env)
    assert {block_key(p) for p in flow_blocks(report)} == blocks, report
    pairs = {(block_key(p), h) for p in flow_blocks(report) for h in p["heights"]}
    ran = set()
    for tile in sorted({h for _, h in pairs}):
        with runtime(blob, dtype, env + (("JU_FLOW_TILE", str(tile)),)) as rt:
            got = run_frames(rt, clip(shape), tensor_names(cfg))
            ran |= check_forced_tile(rt.plan_report(), tile)
        assert_same(got, ref, (shape, path, "JU_FLOW_TILE", tile))
    assert ran == pairs and len({h for _, h in pairs}) >= 6, (sorted(pairs - ran), sorted(pairs))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flow_block_tile_heights_with_leaky_relu(shape, dtype):
    """Case 1, LeakyReLU flow activation (the kernels' other epilogue scale), one height per block: the tallest the
    report lists for it."""
    cfg, _, blob = model(shape, LRELU)
    ref, report = default_run(shape, dtype, LRELU)
    assert {block_key(p) for p in flow_blocks(report)} == FUSED, report
    tallest = {(block_key(p), max(p["heights"])) for p in flow_blocks(report)}
    ran = set()
    for tile in sorted({t for _, t in tallest}):
        with runtime(blob, dtype, (("JU_FLOW_TILE", str(tile)),)) as rt:
            got = run_frames(rt, clip(shape), tensor_names(cfg))
            ran |= check_forced_tile(rt.plan_report(), tile)
        assert_same(got, ref, (shape, "lrelu", tile))
    assert tallest <= ran and len(tallest) == len(FUSED), (tallest, ran)  # (one height for each of the six blocks)


def device_clip(shape, n_out):
    import torch
    dev = torch.device("cuda", 0)
    h, w = SHAPES[shape]
    d_in = torch.from_numpy(clip(shape).copy()).to(dev)
    d_out = torch.zeros((n_out, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return d_in, d_out


AFTER = ("state", "flow_in", "gen_in")  # (a pass computes its flow fields in tensors of its own: what it leaves behind)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flow_block_tile_heights_in_a_lookahead_pass(shape, dtype):
    """Case 2: the same heights in ONE look-ahead pass of three frames (ju_process_batch; grid.z = the frame) -- the
    bytes are those of frame-by-frame ju_process under the default plan."""
    h, w = SHAPES[shape]
    cfg, _, blob = model(shape)
    ref, report = default_run(shape, dtype)
    pairs = {(block_key(p), t) for p in flow_blocks(report) for t in p["heights"]}
    d_in, d_out = device_clip(shape, N_FRAMES)
    ran = set()
    for tile in sorted({t for _, t in pairs}):
        with runtime(blob, dtype, (("JU_FLOW_TILE", str(tile)),)) as rt:
            d_out.zero_()
            rt.process_batch([rt.device_image(d_in[k].data_ptr(), w, h) for k in range(N_FRAMES)],
                             [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(N_FRAMES)])
            assert rt.stat("lookahead_frames") == N_FRAMES, "the call did not take a look-ahead pass"
            ran |= check_forced_tile(rt.plan_report(), tile, items=N_FRAMES)
            frames = d_out.cpu().numpy()
            after = {n: rt.read_tensor(n) for n in AFTER}
        for k in range(N_FRAMES):
            assert np.array_equal(frames[k], ref[k]["frame"]), (shape, "pass", tile, k)
        for n in AFTER:
            assert np.array_equal(after[n], ref[-1][n]), (shape, "pass", tile, n)
    assert ran == pairs, sorted(pairs - ran)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flow_block_tile_heights_in_a_group_pass(shape, dtype):
    """Case 2: the same heights in group passes of two runtimes (ju_process_group; the first block's INDEP
    instantiation, every item with a history of its own).  Runtime a is one frame ahead of b, the lead changes: a sees
    frames 0, 1, 2 and b frames 0, 1 of the clip, and each gives the frames and leaves the tensors of frame-by-frame
    ju_process under the default plan."""
    h, w = SHAPES[shape]
    cfg, _, blob = model(shape)
    ref, report = default_run(shape, dtype)
    heights = sorted({t for p in flow_blocks(report) for t in p["heights"]})
    d_in, d_out = device_clip(shape, 5)
    image = lambda rt, d, s: rt.device_image(d.data_ptr(), s * w, s * h)
    indep = set()
    for tile in heights:
        env = (("JU_FLOW_TILE", str(tile)),)
        with runtime(blob, dtype, env) as a, runtime(blob, dtype, env) as b:
            d_out.zero_()
            a.process(image(a, d_in[0], 1), image(a, d_out[0], 4))
            R.process_group([a, b], [image(a, d_in[1], 1), image(b, d_in[0], 1)], [image(a, d_out[1], 4), image(b, d_out[3], 4)])
            R.process_group([b, a], [image(b, d_in[1], 1), image(a, d_in[2], 1)], [image(b, d_out[4], 4), image(a, d_out[2], 4)])
            assert a.stat("group_frames") == 2 and b.stat("group_frames") == 2, "the calls did not take group passes"
            for rt in (a, b):  # (the lead's launchers ran the pass: the two reports together)
                ran = check_forced_tile(rt.plan_report(), tile, items=2)
                indep |= {(k, t) for k, t in ran if k[6] == 1}
            frames = d_out.cpu().numpy()
            after = [{n: rt.read_tensor(n) for n in AFTER} for rt in (a, b)]
        for k, want in enumerate((0, 1, 2, 0, 1)):
            assert np.array_equal(frames[k], ref[want]["frame"]), (shape, "group", tile, k)
        for n in AFTER:
            assert np.array_equal(after[0][n], ref[2][n]) and np.array_equal(after[1][n], ref[1][n]), (shape, "group", tile, n)
    first = [p for p in flow_blocks(report) if p["pack"] == 1]
    assert len(first) == 1 and indep == {((16, 32, 0, 1, 0, 1, 1), t) for t in first[0]["heights"]}, indep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_residual_tile_form_heights_give_the_residual_kernels_frames(shape, dtype):
    """Case 3: the residual tile form of flow_block_kernel (JU_RES_BLOCK=tile) at both its heights, 14 and 6 rows,
    against res_block_kernel (plain) and the pipelined default, with the generator on its per-block path
    (JU_TOWER=layers).  The three kernels give equal frames and states (what
    test_pipelined_residual_block_kernel_gives_the_plain_kernels_frames demands of two of them); the tile form's two
    heights also give an equal tower output."""
    cfg, _, blob = model(shape)
    layers = (("JU_TOWER", "layers"),)
    names = tensor_names(cfg)
    ref, report = default_run(shape, dtype, (), layers)
    assert any(p["kernel"] == "res_block_pipe" for p in report) and not flow_blocks(report, outk=(2,)), report
    with runtime(blob, dtype, layers + (("JU_RES_BLOCK", "plain"),)) as rt:
        assert rt.stat("resident_tower") == 0
        got = run_frames(rt, clip(shape), names)
        kernels = {p["kernel"] for p in rt.plan_report()}
    assert "res_block" in kernels and "res_block_pipe" not in kernels, kernels
    assert_same(got, ref, (shape, "plain"))
    trunks = {}
    for tile in (14, 6):
        with runtime(blob, dtype, layers + (("JU_RES_BLOCK", "tile"), ("JU_FLOW_TILE", str(tile)))) as rt:
            got = run_frames(rt, clip(shape), names + ["trunk"])
            rep = rt.plan_report()
        assert check_forced_tile(rep, tile, outk=(2,)) == {((64, 64, 0, 0, 2, 0, 0), tile)}, rep
        assert not {"res_block", "res_block_pipe"} & {p["kernel"] for p in rep}, rep
        trunks[tile] = [d.pop("trunk") for d in got]
        assert_same(got, ref, (shape, "tile", tile))
    for a, b in zip(trunks[14], trunks[6]):
        assert np.array_equal(a, b), (shape, "trunk")


SPLITK_ROWS = (2, 4, 6, 8, 12, 14, 16, 18, 34)
NARROW = (("JU_FLOW_WIDE", "0"),)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("rows", [SPLITK_ROWS[0:3], SPLITK_ROWS[3:6], SPLITK_ROWS[6:9]], ids=lambda r: "rows" + "-".join(map(str, r)))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_splitk_plans_give_the_default_bytes(shape, rows, blocks, dtype):
    """Case 4: conv_splitk_kernel with the 128-filter blocks as launches of their own (JU_FLOW_WIDE=0: five layers, one
    of them the pooled form) at a run-time tile height of 2 .. 34 rows -- against the 13 and 15 rows of the coarsest
    level: a tile taller than the image, a last tile of one row, an exact fit -- with one cout block per workgroup, and
    with two where the launcher allows it (the 128-channel layers), for one frame and for a three-frame pass."""
    h, w = SHAPES[shape]
    cfg, _, blob = model(shape)
    ref, report = default_run(shape, dtype, (), NARROW)
    layers = {(p["cin"], p["cout"], p["pool"]) for p in report if p["kernel"] == "conv_splitk"}
    assert layers == {(128, 128, 1), (128, 256, 0), (256, 256, 0), (256, 128, 0), (128, 128, 0)}, report
    d_in, d_out = device_clip(shape, N_FRAMES)
    for r in rows:
        with runtime(blob, dtype, NARROW + (("JU_SPLITK_PLAN", "%dx%d" % (r, blocks)),)) as rt:
            got = run_frames(rt, clip(shape), tensor_names(cfg))
            rt.reset()
            d_out.zero_()
            rt.process_batch([rt.device_image(d_in[k].data_ptr(), w, h) for k in range(N_FRAMES)],
                             [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(N_FRAMES)])
            assert rt.stat("lookahead_frames") == N_FRAMES
            frames = d_out.cpu().numpy()
            after = {n: rt.read_tensor(n) for n in AFTER}
            rep = [p for p in rt.plan_report() if p["kernel"] == "conv_splitk"]
        for items in (1, N_FRAMES):
            ran = {(p["cin"], p["cout"], p["pool"]): p for p in rep if p["items"] == items}
            assert set(ran) == layers and len(ran) == len([p for p in rep if p["items"] == items]), rep
            for key, p in ran.items():
                # (two cout blocks: the 128-channel layers only -- 256 channels of fragments per wave do not fit)
                assert p["rows"] == r and p["blocks"] == (blocks if key[0] == 128 else 1), ("the forced plan did not run", r, blocks, p)
        assert_same(got, ref, (shape, "split-K", r, blocks))
        for k in range(N_FRAMES):
            assert np.array_equal(frames[k], ref[k]["frame"]), (shape, "split-K pass", r, blocks, k)
        for n in AFTER:
            assert np.array_equal(after[n], ref[-1][n]), (shape, "split-K pass", r, blocks, n)


GENERIC = (("JU_FLOW_CONV", "generic"),)
WIDE_GEN = (("gen_filters", 128),)  # a generator that is not 64 wide: the tower's generic path, 1x1 and 128-channel chunks


def check_conv_forms(rep, nb, rw):
    """conv_mfma_kernel launches of a runtime under JU_CONV_TILE=<nb>x<rw>: every 3x3 layer whose form convTiling
    chooses ran the forced one (a fused pool keeps rw = 2, a fused upsampling rw = 1, 32 couts have no nb = 2; the 1x1
    transposed convolution of the tail is packed for nb = 2 whatever the switch).  Returns the layers that ran it."""
    ran = set()
    for p in rep:
        if p["kernel"] != "conv_mfma" or p["taps"] != 9:
            continue
        if p["cout"] % (32 * nb) == 0:
            assert p["nb"] == nb, ("the forced form did not run", nb, rw, p)
            assert p["rw"] == (2 if p["pool"] else 1 if p["ups"] else rw), ("the forced form did not run", nb, rw, p)
            if p["rw"] == rw:
                ran.add((p["ck"], p["cin"], p["cout"], p["pool"], p["ups"]))
    return ran


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,extra", [(s, ()) for s in sorted(SHAPES)] + [("ragged", WIDE_GEN)],
                         ids=lambda v: v if isinstance(v, str) else ("gen128" if v else "gen64"))
def test_generic_conv_tile_forms_and_staging_depths_give_the_default_bytes(shape, extra, dtype):
    """Case 5: conv_mfma_kernel, one launch per flow layer (JU_FLOW_CONV=generic), in all four (nb, rw) tile forms
    where the layer admits them, and at staging depths 0 / 1 / 2 on the multi-chunk layers; with a 128-filter generator
    the tower's convolutions take the same kernel (64-channel chunks of a 128-channel layer, the 16-channel-chunk head,
    the 1x1 form).  The kernel adds a chunk's taps and k-steps in order, chunk after chunk, into accumulators that
    start at the bias, whatever nb, rw and the staging depth (conv_kernels.hip: convChunkMfma and the two chunk loops of
    conv_mfma_kernel): equality, as for the other kernels."""
    cfg, _, blob = model(shape, extra)
    names = tensor_names(cfg) + ["trunk"]
    base = GENERIC
    with runtime(blob, dtype, base) as rt:
        ref = run_frames(rt, clip(shape), names)
        report = rt.plan_report()
    assert not flow_blocks(report) and not [p for p in report if p["kernel"] == "conv_splitk"], report
    layers3 = {(p["ck"], p["cin"], p["cout"]) for p in report if p["kernel"] == "conv_mfma" and p["taps"] == 9}
    assert {(16, 16, 32), (32, 32, 64), (64, 64, 128), (64, 128, 256), (64, 256, 256), (64, 256, 128)} <= layers3, report
    hw = {(p["H"], p["W"]) for p in report if p["kernel"] == "conv_mfma" and p["taps"] == 9 and p["cin"] == 128 and p["cout"] == 128}
    assert (SHAPES[shape] in hw) == bool(extra), report       # (the generator's own 128 -> 128 layers, at the frame's size)
    assert any(p["kernel"] == "conv_mfma" and p["taps"] == 1 for p in report) == bool(extra), report
    for nb in (1, 2):
        for rw in (1, 2):
            with runtime(blob, dtype, base + (("JU_CONV_TILE", "%dx%d" % (nb, rw)),)) as rt:
                got = run_frames(rt, clip(shape), names)
                ran = check_conv_forms(rt.plan_report(), nb, rw)
            # (the plain 3x3 layers with 64 couts or more: at least the six of the encoder and the decoder's second convs)
            assert len(ran) >= 6, (nb, rw, ran)
            assert_same(got, ref, (shape, "JU_CONV_TILE", nb, rw))
    for stages in (0, 1, 2):
        with runtime(blob, dtype, base + (("JU_CONV_DBUF", str(stages)),)) as rt:
            got = run_frames(rt, clip(shape), names)
            multi = [p for p in rt.plan_report() if p["kernel"] == "conv_mfma" and p["taps"] == 9 and p["ck"] == 64 and
                     p["cin"] > 64 and p["nb"] == 1 and not p["ups"]]
        assert len(multi) >= 4 and all(p["stages"] == stages for p in multi), ("the forced depth did not run", stages, multi)
        assert_same(got, ref, (shape, "JU_CONV_DBUF", stages))


def test_two_runtimes_of_one_process_run_different_plans():
    """The plan switches are read where a runtime is constructed: two runtimes alive at the same time, frames
    interleaved, run the tile heights each was constructed under -- and give the same bytes."""
    cfg, _, blob = model("ragged")
    names = tensor_names(cfg)
    with runtime(blob, R.DTYPE_F16, (("JU_FLOW_TILE", "18"),)) as tall, runtime(blob, R.DTYPE_F16, ()) as plain:
        for f in clip("ragged"):
            a, b = tall.process_image(f).copy(), plain.process_image(f).copy()
            assert np.array_equal(a, b)
            for n in names:
                assert np.array_equal(tall.read_tensor(n), plain.read_tensor(n)), n
        rows = [{block_key(p): p["rows"] for p in flow_blocks(rt.plan_report())} for rt in (tall, plain)]
    assert rows[0][(32, 64, 0, 1, 0, 0, 0)] == 18 and rows[1][(32, 64, 0, 1, 0, 0, 0)] != 18, rows
    assert set(rows[0]) == set(rows[1]) == FUSED


@functools.lru_cache(maxsize=None)
def oracle_run(shape, n):
    """The float64 oracle's first n frames at a shape (a few seconds per frame on the CPU): once, for both dtypes."""
    cfg, wts, _ = model(shape)
    sess = O.Session(wts, oracle_config(cfg))
    out = []
    for f in clip(shape)[:n]:
        trace = {}
        frame = sess.run(f, trace)
        out.append((frame, trace["flow"], np.array(sess.last.output_raw), trace["gen_in_ref"]))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["exact", "ragged"])
def test_default_plan_matches_the_oracle(shape, dtype):
    """What the plans above are compared WITH: the default plan at the two new shapes against the float64 oracle, two
    frames, the suite's tolerances (gpu_common.py: u8 frame, flow head, output_raw, generator input)."""
    h, w = SHAPES[shape]
    oc = oracle_config(config(shape))
    got, _ = default_run(shape, dtype)
    for t, (frame, flow, raw, gen_in) in enumerate(oracle_run(shape, 2)):
        check_u8(got[t]["frame"], frame, dtype, ("launch-plans", shape, t))
        tol = TOL[dtype]
        e = err(got[t]["flow"].reshape(oc.padded_height, oc.padded_width, 32), flow)["max_abs"]
        assert e <= tol["flow"], (shape, t, "flow", e)
        e = err(got[t]["state"].reshape(4 * h, 4 * w, 4)[..., :3], raw)["max_abs"]
        assert e <= tol["raw"], (shape, t, "output_raw", e)
        e = err(gen_in_to_reference(got[t]["gen_in"], h, w), gen_in)["max_abs"]
        assert e <= tol["raw"], (shape, t, "gen_in", e)
