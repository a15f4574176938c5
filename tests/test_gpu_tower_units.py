"""The resident tower's fast schedule in its row-quad form (tower_resident_kernel, UROWS = 4) against its row-pair
form and the plain schedule (debug variant 8).  All three execute the same sequence of MFMAs per accumulator, take
the bias as the C operand of the first ones and apply the same epilogue expression, so frames, state and trunk must
be EQUAL: a lost halo row, a fragment register used before its read landed, a deferred group written to the wrong
row or a weight register refilled too early shows as a difference (or as a bounded-wait fallback), never as a hang.

The frames are the smallest that reach every position a quad can be in:

    32x64   regions 2x2, all 16 rows          every region at an image corner
    46x64   rows 16 / 16 / 14                 the two-row tail unit; a region with neighbours above and below
    48x96   regions 3x3, all 16 rows          one region with all eight neighbours
    62x32   one column, 16 / 16 / 16 / 14     left and right image border in the same region
    36x64   rows 12 / 12 / 12                 no interior quad for parity 0: the pair form, still the fast schedule
    44x64   rows 15 / 15 / 14                 (three regions of ceil(44 / 3) rows: an odd height) the general schedule

44x64 was meant to give 16 / 16 / 12; the geometry balances the region rows instead (residentTowerGeometry), so that
frame reports tower_fast = 0 and tower_unit_rows = 2.  36x64 is the frame that has 12-row regions on the fast schedule.
"""

import numpy as np
import pytest

from helpers import small_config
from joshupscale_amd import model_file as M
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

# (height, width): (unit rows the default takes, tower_fast)
SHAPES = {
    (32, 64): (4, 1),
    (46, 64): (4, 1),
    (48, 96): (4, 1),
    (62, 32): (4, 1),
    (36, 64): (2, 1),
    (44, 64): (2, 0),
}
FRAMES = 4


def model(h, w):
    cfg = small_config(frame_height=h, frame_width=w, gen_blocks=3)
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    return blob, M.synthetic_frames(FRAMES, h, w, seed=11, kind="noise")


def run_schedule(lib, blob, frames, dtype, schedule, expect_rows, expect_fast):
    """schedule: 4 = the default, 2 = row pairs forced, 8 = the plain schedule -> (frames, state, trunk)"""
    lib.ju_debug_set(b"tower_variant", 8 if schedule == 8 else 0)
    lib.ju_debug_set(b"tower_unit_rows", 2 if schedule == 2 else 4)
    try:
        with R.Runtime(blob, 0, dtype) as rt:
            assert rt.stat("resident_tower") == 1
            assert rt.stat("tower_variant") == (8 if schedule == 8 else 0)
            assert rt.stat("tower_fast") == expect_fast
            assert rt.stat("tower_unit_rows") == (expect_rows if schedule != 2 else 2)
            outs = [rt.process_image(f).copy() for f in frames]
            state = rt.read_tensor("state").copy()
            trunk = rt.read_tensor("trunk").copy()
            assert rt.stat("fallbacks") == 0
        return outs, state, trunk
    finally:
        lib.ju_debug_set(b"tower_variant", 0)
        lib.ju_debug_set(b"tower_unit_rows", 4)


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=["%dx%d" % s for s in SHAPES])
def test_row_quads_do_not_change_the_bytes(shape, dtype, monkeypatch):
    monkeypatch.setenv("JU_TAIL", "fused")   # (every schedule writes the trunk; the tail runs as a launch of its own)
    lib = R.load_library()
    rows, fast = SHAPES[shape]
    blob, frames = model(*shape)
    got = {s: run_schedule(lib, blob, frames, dtype, s, rows, fast) for s in (4, 2, 8)}
    for other in (2, 8):
        assert np.array_equal(got[4][2], got[other][2]), ("trunk", shape, other)
        assert np.array_equal(got[4][1], got[other][1]), ("state", shape, other)
        for t, (a, b) in enumerate(zip(got[4][0], got[other][0])):
            assert np.array_equal(a, b), ("frame", t, shape, other)


@pytest.mark.parametrize("dtype", [R.DTYPE_BF16, R.DTYPE_F16], ids=["bf16", "f16"])
def test_row_quads_in_a_look_ahead_pass(dtype):
    """Four frames of 46x64 as ONE look-ahead pass (ju_process_batch, the product's fused tail) against the same
    frames one per call, both on row quads."""
    import torch
    h, w = 46, 64
    lib = R.load_library()
    lib.ju_debug_set(b"tower_unit_rows", 4)
    blob, frames = model(h, w)
    d_in = torch.from_numpy(frames).to("cuda:0")
    d_out = torch.zeros((FRAMES, 4 * h, 4 * w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with R.Runtime(blob, 0, dtype) as rt:
        assert rt.stat("tower_fast") == 1 and rt.stat("tower_unit_rows") == 4
        single = [rt.process_image(f).copy() for f in frames]
        state = rt.read_tensor("state").copy()
        assert rt.stat("fallbacks") == 0
    with R.Runtime(blob, 0, dtype) as rt:
        rt.process_batch([rt.device_image(d_in[k].data_ptr(), w, h) for k in range(FRAMES)],
                         [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(FRAMES)])
        assert rt.stat("lookahead_frames") == FRAMES
        assert rt.stat("tower_unit_rows") == 4 and rt.stat("fallbacks") == 0
        assert np.array_equal(rt.read_tensor("state"), state)
    got = d_out.cpu().numpy()
    for t in range(FRAMES):
        assert np.array_equal(got[t], single[t]), t
