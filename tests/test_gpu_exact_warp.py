"""warp_pack_kernel alone on the GPU (ju_debug_warp) against its exact definition (tests/exact_reference.py warp;
docs/exact_tests.md): f16 flows that are multiples of 1/8 and f16 states that are multiples of 2^-9 in [-0.5, 0.5] make
both interpolations exact in f32, so every slot of every record, every pre_warp value and every byte of the output_flow
frame must EQUAL the reference's.  Slots 12 .. 14 (x / 255 - 0.5, not dyadic) accept the two neighbouring words at the byte
values where correct f32 evaluations differ (one of 256 in bf16, none in f16).  The table: tests/exact_cases.py WARP_CASES,
checked without a GPU in test_exact_cpu.py.  Guard bytes surround every buffer and fill the padding of pitched ones; the
record tensor in the tower layout keeps its zero border."""

import ctypes as C

import numpy as np
import pytest

import exact_cases as K
import exact_reference as E
from joshupscale_amd import runtime as R
from test_gpu_exact_conv import BAND, GUARD, DevTensor, Tally, ids, launched, torch_dev

pytestmark = pytest.mark.gpu


class DevBytes:
    """Rows of bytes on the device between guard bands: `pad` guard bytes behind each row, row 0 `offset` bytes past a
    256-byte boundary, bottom-up when `flip`."""

    def __init__(self, rows, row_bytes, pad=0, offset=0, flip=False, fill=None):
        self.rows, self.row_bytes, self.pitch, self.lead, self.flip = rows, row_bytes, row_bytes + pad, BAND + offset, flip
        self.host = np.full(self.lead + rows * self.pitch + BAND, GUARD, np.uint8)
        if fill is not None:
            self._rows(self.host)[...] = np.asarray(fill, np.uint8).reshape(rows, row_bytes)
        torch, dev = torch_dev()
        self.buf = torch.from_numpy(self.host.copy()).to(dev)

    def _rows(self, buf):
        body = buf[self.lead:self.lead + self.rows * self.pitch].reshape(self.rows, self.pitch)[:, :self.row_bytes]
        return body[::-1] if self.flip else body

    @property
    def ptr(self):
        base = self.buf.data_ptr() + self.lead
        return base + (self.rows - 1) * self.pitch if self.flip else base

    @property
    def stride(self):
        return -self.pitch if self.flip else self.pitch

    def read(self):
        got = self.buf.cpu().numpy()
        rows = self._rows(got).copy()
        expect = self.host.copy()
        self._rows(expect)[...] = rows
        assert np.array_equal(got, expect), "guard bytes changed"
        return rows


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
@pytest.mark.parametrize("case", K.WARP_CASES, ids=ids(K.WARP_CASES))
def test_warp_pack_is_exact_on_dyadic_inputs(case, dtype):
    lib = R.load_library(True)
    H, W = case["H"], case["W"]
    d, ref = K.warp_reference(case, dtype)
    state = DevTensor(1, 4 * H, 4 * W, 4, fill=E.rne(d["state"], E.F16)).upload()
    flow = DevTensor(1, d["PH"], d["PW"], 32, fill=E.rne(d["flow"], E.F16)).upload()
    frame = DevBytes(H, 4 * W, pad=12, offset=4, fill=d["frame"])
    out = DevTensor(1, H, W, 64, tower=case["tower_pitch"]).upload()
    pre = DevTensor(1, 4 * H, 4 * W, 4).upload() if case["pre_warp"] else None
    u8 = None
    if case["out_u8"] is not None:
        pad, offset, flip = case["out_u8"]
        u8 = DevBytes(4 * H, 16 * W, pad=pad, offset=offset, flip=flip)
    a = R.JuDebugWarp()
    a.dtype, a.state, a.flow, a.frame, a.frame_stride, a.out = dtype, state.ptr, flow.ptr, frame.ptr, frame.stride, out.ptr
    a.out_pitch, a.H, a.W, a.PW, a.pad_top, a.pad_left = out.pitch if case["tower_pitch"] else 0, H, W, d["PW"], case["pads"][0], case["pads"][1]
    a.sums, a.pre_warp_out = None, pre.ptr if pre else None
    a.out_u8, a.out_stride = (u8.ptr, u8.stride) if u8 else (None, 0)
    launched(lib.ju_debug_warp(C.byref(a)))
    what = (case["name"], K.DTYPE_NAMES[dtype])
    tally = Tally()
    got = out.read()[0]
    tally.compare(got, dict(words=ref["records"], exact=ref["exact"], out_type=dtype), what + ("records",), alt=ref["records_alt"])
    if pre is not None:
        tally.compare(pre.read()[0], dict(words=ref["pre_warp"], exact=ref["exact"], out_type=E.F16), what + ("pre_warp",))
    if u8 is not None:
        rows = u8.read().reshape(4 * H, 4 * W, 4)
        assert np.array_equal(rows, ref["bgrx"]), (what, "output_flow frame", np.argwhere(rows != ref["bgrx"])[:8])
    for t in (state, flow):
        t.unchanged()
    assert np.array_equal(frame.buf.cpu().numpy(), frame.host)
    tally.finish((case["name"],), dtype, case["field"] == "fractions")
