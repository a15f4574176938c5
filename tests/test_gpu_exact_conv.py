"""The network's convolution, flow-block and resampling kernels alone on the GPU (ju_debug_conv, ju_debug_flow_block,
ju_debug_resample) against exact integer arithmetic plus ONE rounding (tests/exact_reference.py; docs/exact_tests.md): the
inputs are dyadic, so the summation order cannot matter and every output word must EQUAL the reference's -- no tolerance
(the two zeros are not told apart).  The tables and their dyadic condition: tests/exact_cases.py, checked without a GPU in
test_exact_cpu.py.

Every device buffer lies between guard bands of a fixed byte, pitched tensors carry the byte in their padding columns and
items in the gaps between them: all of it has to come back untouched.  A tower-layout tensor's border and surplus rows and
columns are zero instead and have to stay zero.  Each test records the zeros mapped, the outputs the final rounding
changed and the exact ties among them (gpu_common.record: the session's parity statistics), and where a case is meant to round the last two are
not zero."""

import ctypes as C
import re

import numpy as np
import pytest

import exact_cases as K
import exact_reference as E
from gpu_common import record
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

GUARD = 0xA5
BAND = 256                                                # guard bytes in front of and behind every buffer


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


class DevTensor:
    """`items` tensors [rows][width][ch] of 16-bit words on the device, `pitch` pixels per row, `gap` guard bytes behind each
    item, the whole between two guard bands.  tower: each item is a tower-layout allocation [tower_rows][tower_pitch][ch] of
    zeros with the image at row / column 1, and `ptr` is the image's pixel (0, 0)."""

    def __init__(self, items, rows, width, ch, pitch=0, gap=0, tower=False, fill=None):
        self.items, self.rows, self.width, self.ch, self.tower = items, rows, width, ch, tower
        if tower:
            self.prows, self.pitch, self.oy, self.ox = K.tower_rows(rows), K.tower_pitch(width), 1, 1
        else:
            self.prows, self.pitch, self.oy, self.ox = rows, pitch or width, 0, 0
        self.body = self.prows * self.pitch * ch * 2
        self.item_bytes = self.body + gap
        self.host = np.full(BAND + items * self.item_bytes + BAND, GUARD, np.uint8)
        if tower:
            for i in range(items):
                self._body(self.host, i)[...] = 0
        if fill is not None:
            self.put(fill)
        self.buf = None

    def _body(self, buf, i):
        start = BAND + i * self.item_bytes
        return buf[start:start + self.body].view(np.uint16).reshape(self.prows, self.pitch, self.ch)

    def _image(self, buf, i):
        return self._body(buf, i)[self.oy:self.oy + self.rows, self.ox:self.ox + self.width]

    def put(self, words):
        words = np.asarray(words, np.uint16).reshape(self.items, self.rows, self.width, self.ch)
        for i in range(self.items):
            self._image(self.host, i)[...] = words[i]
        return self

    def upload(self):
        torch, dev = torch_dev()
        self.buf = torch.from_numpy(self.host.copy()).to(dev)
        assert self.buf.data_ptr() % 256 == 0
        return self

    @property
    def ptr(self):
        return self.buf.data_ptr() + BAND + ((self.oy * self.pitch + self.ox) * self.ch) * 2

    def read(self):
        """The items' words as the device holds them; every byte around them must be what was uploaded."""
        got = self.buf.cpu().numpy()
        words = np.stack([self._image(got, i).copy() for i in range(self.items)])
        expect = self.host.copy()
        for i in range(self.items):
            self._image(expect, i)[...] = words[i]
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, ("guard bytes, padding or zero border changed", bad[:8], got[bad[:8]], expect[bad[:8]])
        return words

    def unchanged(self):
        got = self.buf.cpu().numpy()
        assert np.array_equal(got, self.host), "an input buffer changed"


class Tally:
    """The three counts of a test, and the comparison that feeds them."""

    def __init__(self):
        self.zeros = self.changed = self.ties = self.elements = self.launches = 0

    def compare(self, got, ref, what, alt=None):
        """got, ref: words; ref's `exact` and `out_type` give the rounding counts.  Equality after folding -0 into +0."""
        want, z_want = E.fold_zero(ref["words"])
        have, z_have = E.fold_zero(got)
        ok = have == want
        if alt is not None:
            ok |= have == E.fold_zero(alt)[0]
        if not ok.all():
            bad = np.argwhere(~ok)
            first = tuple(bad[0])
            raise AssertionError((what, "%d of %d words differ" % (len(bad), ok.size), "first at", first, "got", hex(int(have[first])),
                                  "want", hex(int(want[first])), "rows", sorted(set(bad[:, 0].tolist()))[:12], "columns",
                                  sorted(set(bad[:, 1].tolist()))[:12], "channels", sorted(set(bad[:, -1].tolist()))[:12]))
        c, t = E.rounding_counts(ref["exact"], ref["out_type"])
        self.zeros += z_want + z_have
        self.changed += c
        self.ties += t
        self.elements += ok.size
        self.launches += 1

    def finish(self, what, dtype, rounds):
        record(("exact",) + tuple(what), dtype, dict(zeros_mapped=self.zeros, rounded=self.changed, ties=self.ties,
                                                     elements=self.elements, launches=self.launches))
        if rounds:
            assert self.changed > 0 and self.ties > 0, (what, self.changed, self.ties)


def plan_of(**kw):
    p = R.JuDebugPlan(0, 0, -1, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def launched(rc):
    """A hook's return code: a device error ends the session (nothing more is started on a GPU that has faulted)."""
    if rc != 0:
        msg = R.load_library(True).ju_last_error().decode(errors="replace")
        if msg.startswith("HipException"):
            pytest.exit("device error, session ended: " + msg, returncode=3)
        raise AssertionError(msg)


def call(fn, args):
    lib = R.load_library(True)
    text = C.create_string_buffer(4096)
    args.plan_text = C.cast(text, C.c_void_p)
    args.plan_capacity = len(text)
    launched(getattr(lib, fn)(C.byref(args)))
    return text.value.decode()


def plan_fields(text):
    lines = text.strip().splitlines()
    assert len(lines) == 1, text
    return lines[0].split()[0], {k: v for k, v in re.findall(r"(\w+)=(\S+)", lines[0])}


# ---- convolutions -------------------------------------------------------------------------------------------------------------
def run_conv(case, shape_index, dtype, tally):
    h, w = case["shapes"][shape_index]
    act = K.act_of(case, shape_index)
    d, refs = K.conv_reference(case, shape_index, act, dtype)
    ih, iw = d["x"].shape[1:3]
    oh, ow = refs[0]["words"].shape[:2]
    tower = case["tower"]
    x = DevTensor(case["items"], ih, iw, case["cin"], iw + case["in_pad"] if case["in_pad"] else 0, case["gap"], tower,
                  fill=E.rne(d["x"], dtype)).upload()
    out = DevTensor(case["items"], oh, ow, case["cout"], ow + case["out_pad"] if case["out_pad"] else 0, case["gap"], tower).upload()
    res = None
    if d["res"] is not None:
        res = DevTensor(1, h, w, case["cout"], w + case["res_pad"] if case["res_pad"] else 0, 0, tower, fill=E.rne(d["res"], dtype)).upload()
    wts, bias = f32(d["w"]), f32(d["bias"])
    a = R.JuDebugConv()
    a.kernel, a.dtype, a.inp, a.out, a.res = case["kernel"], dtype, x.ptr, out.ptr, res.ptr if res else None
    a.weights, a.bias = wts.ctypes.data, bias.ctypes.data
    a.H, a.W, a.cin, a.cin_real, a.cout, a.taps, a.relu, a.slope = h, w, case["cin"], case["cin_real"], case["cout"], case["taps"], act, K.SLOPE
    a.out_head, a.pool, a.upsample, a.nb, a.rw = case["out_head"], case["pool"], case["upsample"], case["nb"], case["rw"]
    if tower:
        a.in_pitch = a.out_pitch = a.res_pitch = K.tower_pitch(w)
    else:
        a.in_pitch = x.pitch if case["in_pad"] else 0
        a.out_pitch = out.pitch if case["out_pad"] else 0
        a.res_pitch = res.pitch if res is not None and case["res_pad"] else 0
    a.items, a.in_item_bytes, a.out_item_bytes = case["items"], x.item_bytes, out.item_bytes
    a.plan = plan_of(**case["plan"])
    text = call("ju_debug_conv", a)
    what = (case["name"], "%dx%d" % (h, w), "act%d" % act, K.DTYPE_NAMES[dtype])
    if case["kernel"] != 2:                                # (the tower kernel has no plan and notes none)
        kind, f = plan_fields(text)
        assert kind == ("conv_splitk" if case["kernel"] == 1 else "conv_mfma"), text
        assert (int(f["H"]), int(f["W"]), int(f["cin"]), int(f["cout"]), int(f["items"])) == (h, w, case["cin"], case["cout"], case["items"]), text
        for k, v in case["expect"].items():
            assert int(f[k]) == v, (what, "the forced plan did not run", text)
        if case["kernel"] == 0:
            assert (int(f["nb"]), int(f["rw"]), int(f["taps"])) == (case["nb"], case["rw"], case["taps"]), text
    else:
        assert text == "", text
    got = out.read()
    x.unchanged()
    if res is not None:
        res.unchanged()
    for i in range(case["items"]):
        tally.compare(got[i], refs[i], what + ("item%d" % i,))


def conv_test(case, dtype):
    tally = Tally()
    for si in range(len(case["shapes"])):
        run_conv(case, si, dtype, tally)
    tally.finish((case["name"],), dtype, dtype in case["rounds"])


def ids(cases):
    return [c["name"] for c in cases]


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
@pytest.mark.parametrize("case", K.CONV_CASES, ids=ids(K.CONV_CASES))
def test_conv_mfma_is_exact_on_dyadic_inputs(case, dtype):
    conv_test(case, dtype)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
@pytest.mark.parametrize("case", K.SPLITK_CASES, ids=ids(K.SPLITK_CASES))
def test_conv_splitk_is_exact_on_dyadic_inputs(case, dtype):
    conv_test(case, dtype)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
@pytest.mark.parametrize("case", K.TOWER_CASES, ids=ids(K.TOWER_CASES))
def test_conv_tower_is_exact_on_dyadic_inputs(case, dtype):
    conv_test(case, dtype)


# ---- flow blocks --------------------------------------------------------------------------------------------------------------
def run_flow_block(case, th, shape, items, act, dtype, tally):
    h, w = shape
    d, refs = K.fb_reference(case, shape, items, act, dtype)
    ih, iw = d["x"].shape[1:3]
    oh, ow = refs[0]["words"].shape[:2]
    tower = case["tower"]
    x = DevTensor(items, ih, iw, case["cin"], 0 if tower or w % 4 != 2 else iw + 2, 32 if items > 1 else 0, tower,
                  fill=E.rne(d["x"], dtype)).upload()
    out = DevTensor(items, oh, ow, case["cmid"], 0 if tower or h % 4 else ow + 3, 48 if items > 1 else 0, tower).upload()
    w1, b1, w2, b2 = f32(d["w1"]), f32(d["b1"]), f32(d["w2"]), f32(d["b2"])
    a = R.JuDebugFlowBlock()
    a.dtype, a.inp, a.out = dtype, x.ptr, out.ptr
    a.weights1, a.bias1, a.weights2, a.bias2 = w1.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data
    a.H, a.W, a.cin, a.cin_real, a.cmid = h, w, case["cin"], case["cin_real"], case["cmid"]
    a.upsample, a.pool, a.out_head, a.residual = case["upsample"], case["pool"], case["out_head"], case["residual"]
    a.act1, a.act2, a.slope = act, act, K.SLOPE
    a.in_pitch = x.pitch if tower or x.pitch != iw else 0
    a.out_pitch = out.pitch if tower or out.pitch != ow else 0
    a.items, a.in_item_bytes, a.out_item_bytes = items, x.item_bytes, out.item_bytes
    a.plan = plan_of(flow_tile=th if case["form"] == "flow_block" else 0, **case["plan"])
    text = call("ju_debug_flow_block", a)
    what = (case["name"], "rows%d" % th, "%dx%d" % (h, w), "items%d" % items, "act%d" % act, K.DTYPE_NAMES[dtype])
    kind, f = plan_fields(text)
    assert kind == case["form"], (what, text)
    assert (int(f["H"]), int(f["W"])) == (h, w), text
    heights = None
    if kind == "flow_block":
        heights = [int(v) for v in f["heights"].split(",")]
        assert set(heights) <= set(case["all_heights"]) and int(f["items"]) == items, text
        if th in heights:
            assert int(f["rows"]) == th, (what, "the forced tile height did not run", text)
    got = out.read()
    x.unchanged()
    for i in range(items):
        tally.compare(got[i], refs[i], what + ("item%d" % i,))
    return heights


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
@pytest.mark.parametrize("case", K.FB_CASES, ids=ids(K.FB_CASES))
def test_flow_block_is_exact_on_dyadic_inputs(case, dtype):
    tally = Tally()
    ran, has = set(), set()
    for k, (th, shape, items) in enumerate(K.fb_runs(case)):
        act = case["acts"][k % len(case["acts"])]
        heights = run_flow_block(case, th, shape, items, act, dtype, tally)
        if heights is not None:
            has |= set(heights)
            if th in heights:
                ran.add(th)
    # every tile height the shape has was forced and ran (a wide case runs the shortest alone; the res-block kernels have one)
    if case["form"] == "flow_block" and not case["wide"]:
        assert ran == has and has, (case["name"], ran, has)
    tally.finish((case["name"],), dtype, dtype in case["rounds"])


# ---- upsample2 / maxpool2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
@pytest.mark.parametrize("case", K.RESAMPLE_CASES, ids=ids(K.RESAMPLE_CASES))
def test_resampling_is_exact(case, dtype):
    tally = Tally()
    lib = R.load_library(True)
    for size in case["sizes"]:
        xs, refs = K.resample_reference(case, size, dtype)
        h, w = size
        oh, ow = refs[0][0].shape[:2]
        x = DevTensor(case["items"], h, w, case["C"], fill=E.rne(xs, dtype)).upload()
        out = DevTensor(case["items"], oh, ow, case["C"]).upload()
        a = R.JuDebugResample(case["op"], dtype, x.ptr, out.ptr, h, w, case["C"], case["items"])
        launched(lib.ju_debug_resample(C.byref(a)))
        got = out.read()
        x.unchanged()
        for i in range(case["items"]):
            tally.compare(got[i], dict(words=refs[i][0], exact=refs[i][1], out_type=dtype), (case["name"], size, i))
    tally.finish((case["name"],), dtype, dtype in case["rounds"])
