"""The temporal output filter alone on the GPU (ju_debug_temporal: zero_words_kernel, temporal_reduce_kernel,
temporal_blend_kernel) against its definition (tests/temporal_reference.py; the table's conditions and its sensitivity
are checked without a GPU in test_temporal_cpu.py):

 1. reduce: every accumulator the run returned / 2^32 against the float64 sum, to 2^-16 of the window's sum of |term| (plus
    2^-16 per term with brightness); the words behind the window grid zero; a second run bit for bit the same;
 2. gate + blend: from the accumulators this run returned, every byte and every state element in its acceptance interval;
 3. a global hard cut leaves the state and the frame as they were passed in;
 4. constructed cases in which every operation is exact;
 5. two runs of the largest case agree in every byte.
Around every buffer lie guard bytes that have to come back untouched; X is 0."""

import ctypes as C

import numpy as np
import pytest

import temporal_reference as T
from gpu_common import record
from joshupscale_amd import runtime as R
from test_gpu_yuv import DevPlane, torch_dev

pytestmark = pytest.mark.gpu

LAYOUTS = {"dense": dict(pad=0, flip=False), "padded": dict(pad=128, flip=False), "bottom-up": dict(pad=64, flip=True)}
SENTINEL = 0x5A
EXTRA_WORDS = 8                                           # accumulator words read back behind the window grid


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


class Buffers:
    """The device buffers of one run, each inside guard bytes."""

    def __init__(self, case, data, layout):
        torch, _ = torch_dev()
        hh, ww = 4 * case["h"], 4 * case["w"]
        self.hh, self.ww, self.data = hh, ww, data
        self.state = DevPlane(as_bytes(data["state"]))
        self.pre = DevPlane(as_bytes(data["pre_warp"]))
        self.before = np.full((hh, ww * 4), SENTINEL, np.uint8)
        self.out = DevPlane(self.before, **LAYOUTS[layout])
        self.sums = DevPlane(as_bytes(data["sums"][None, :])) if data["sums"] is not None else None
        torch.cuda.synchronize()

    def run(self, case, run):
        lib = R.load_library(True)
        _, _, gh, gw, _, _ = T.geometry(case["h"], case["w"], run["window"])
        acc = np.full(gh * gw + EXTRA_WORDS, 0x1111111111111111, np.uint64)
        rc = lib.ju_debug_temporal(self.state.ptr, self.pre.ptr, self.out.ptr, self.out.stride, self.sums.ptr if self.sums else None,
                                   case["w"], case["h"], run["strength"], run["threshold"], run["gain"], run["window"], T.flags_of(run),
                                   acc.ctypes.data_as(C.c_void_p), acc.size)
        assert rc == 0, lib.ju_last_error()
        state = self._rows(self.state).view(np.float16).reshape(self.hh, self.ww, 4)
        out = self._rows(self.out).reshape(self.hh, self.ww, 4)
        # the guard bytes of the buffers written, every byte of the buffers read
        self.state.check(as_bytes(state))
        self.out.check(as_bytes(out))
        self.pre.check(as_bytes(self.data["pre_warp"]))
        if self.sums:
            self.sums.check(as_bytes(self.data["sums"][None, :]))
        return acc, out, state

    @staticmethod
    def _rows(plane):
        return np.ascontiguousarray(plane._rows(plane.buf.cpu().numpy()))


CASE_IDS = [c["name"] for c in T.CASES]


@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_every_mode_of_a_case_meets_the_definition(case):
    data = T.build(case)
    worst = dict(acc_dev_over_tol=0.0, acc_dev_rel=0.0, byte_off_centre=0.0, state_off_centre=0.0, hard_cuts=0, runs=0)
    for run in T.runs(case, data):
        d = T.define(data["state"], data["pre_warp"], data["sums"], case["h"], case["w"], run)
        bufs = Buffers(case, data, case["layout"])
        acc, out, state = bufs.run(case, run)
        fails, fig = T.check_run(case, data, d, run, acc, out, state, bufs.before.reshape(out.shape))
        print(case["name"], run, fig)
        assert not fails, (case["name"], run, fails, fig)
        if case is not T.BIG:                             # integer sums: a second run gives the same words
            again, _, _ = Buffers(case, data, case["layout"]).run(case, run)
            assert np.array_equal(acc, again), (case["name"], run)
        for k in ("acc_dev_over_tol", "acc_dev_rel", "byte_off_centre", "state_off_centre"):
            worst[k] = max(worst[k], fig.get(k, 0.0))
        worst["hard_cuts"] += fig.get("hard_cut", 0)
        worst["runs"] += 1
    record(("temporal-alone", case["name"]), R.DTYPE_F16, worst)
    if case["window"] == 0 and any(m["gain"] == 0 for m in case["modes"]):
        assert 0 < worst["hard_cuts"] < worst["runs"]     # the global hard cut was met, and so was its opposite


def exact_case(h, w, window, layout, equal):
    hh, ww = 4 * h, 4 * w
    rng = np.random.default_rng(h * 100 + window)
    state = np.zeros((hh, ww, 4), np.float16)
    pre = np.zeros((hh, ww, 4), np.float16)
    if equal:                                             # state = pre_warp: every term 0, acc = 0, c = 0 at threshold 0
        state[..., :3] = rng.uniform(-0.5, 0.5, (hh, ww, 3)).astype(np.float16)
        pre[..., :3] = state[..., :3]
        thr = 0.0
    else:                                                 # |0 - 0.25| everywhere: the mean is the threshold 0.25 itself
        pre[..., :3] = 0.25
        thr = 0.25
    state[..., 3] = 1.0
    pre[..., 3] = -1.0
    case = dict(name="exact", h=h, w=w, window=window, layout=layout)
    run = dict(l2=0, limit=0, luma=0, gain=0.0, window=window, strength=0.5, threshold=thr)
    return case, dict(state=state, pre_warp=pre, sums=None, b=0.0), run


@pytest.mark.parametrize("equal", [False, True], ids=["mean-is-threshold", "state-is-pre_warp"])
@pytest.mark.parametrize("h,w,window", [(5, 7, 0), (16, 16, 0), (16, 16, 16), (16, 16, 64), (4, 8, 1), (30, 48, 24)])
def test_constructed_cases_are_exact(h, w, window, equal):
    # (every window of these geometries is full: no padding, so the windowed means are the threshold too)
    case, data, run = exact_case(h, w, window, "padded", equal)
    acc, out, state = Buffers(case, data, "padded").run(case, run)
    hh, ww, gh, gw, py, px = T.geometry(h, w, window)
    assert (py, px) == (0, 0) and gh * (window or hh) == hh and gw * (window or ww) == ww
    per_cell = 3 * (hh * ww if window == 0 else window * window)
    want_acc = 0 if equal else per_cell * 2 ** 30        # 0.25 per term in 32.32
    assert (acc[:gh * gw] == want_acc).all() and not acc[gh * gw:].any(), acc[:4]
    # c = 0: out = p s / 2 + gen (1 - s / 2) with s = 0.5 -- p / 4 + 3 gen / 4, exact in f32 for f16 inputs
    r = data["pre_warp"][..., :3].astype(np.float64) * 0.25 + data["state"][..., :3].astype(np.float64) * 0.75
    assert np.array_equal(r.astype(np.float16).astype(np.float64), r)
    assert np.array_equal(state[..., :3].view(np.uint16), r.astype(np.float16).view(np.uint16))
    assert not state[..., 3].view(np.uint16).any()
    assert np.array_equal(out[..., :3], T.to_byte(r)) and not out[..., 3].any()
    if not equal:
        assert (out[..., :3] == 143).all() and (state[..., :3] == np.float16(0.0625)).all()


def test_two_runs_of_the_largest_case_agree_in_every_byte():
    case = T.BIG
    data = T.build(case)
    run = T.runs(case, data)[0]
    first = Buffers(case, data, case["layout"]).run(case, run)
    second = Buffers(case, data, case["layout"]).run(case, run)
    assert np.array_equal(first[0], second[0])
    assert np.array_equal(first[1], second[1])
    assert np.array_equal(first[2].view(np.uint16), second[2].view(np.uint16))
