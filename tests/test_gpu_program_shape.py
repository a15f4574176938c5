"""The per-frame program of every model form and every path switch, pinned by its shape -- needs an MI355X.

The engine's program builder (csrc/engine_program.cpp) decides which launches a frame runs.  This file holds what it
decides: for every case below the number of launches per frame, whether the generator's and the flow net's towers are
resident, and for every step tag the pair (launches, flops), with the flops of every single `flow` and `tower` launch
-- compared with `==` against tests/golden/program_shapes.json.  Every flops value is a product of small integers far
below 2^53, exact in a double whatever the multiplication order: a mismatch is a real difference.

Nothing is launched: Runtime.time_steps(tag, 0) returns (0.0, launches, flops) of the program as built.

The golden file was recorded from the library BEFORE the builder was split into stages (JU_RECORD_PROGRAM_SHAPES=1
writes it) and is not to be recorded again from a builder that was edited since: a difference is a finding about the
builder, not about the file.  A PR that adds a launch on purpose states the new figures in its own diff of the file.

Cases, all at 30x48 with two generator blocks:
  (a) eleven models under no switch, in bf16 and f16
  (b) the default model in bf16 under each path switch alone; the 64-filter flow-resnet under JU_FLOW=layers / convs
  (c) the 8-bit engine on the default model under no switch, JU_TOWER=layers and JU_TOWER=convs
"""

import contextlib
import functools
import json
import os

import pytest

from flowfree_common import flow_free
from helpers import M, ROOT, small_config
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "program_shapes.json")
TAGS = ("lr_pack", "pack", "flow", "warp", "calib", "gen_head", "tower", "tail", "temporal")
STATS = ("launches_per_frame", "resident_tower", "resident_flow")
# every switch that selects a path of the program: a case states the one it wants, the rest is unset
SWITCHES = ("JU_TOWER", "JU_TAIL", "JU_PACK", "JU_POOL", "JU_UPSAMPLE", "JU_FLOW_CONV", "JU_CALIBRATE", "JU_FLOW")
GEN_BLOCKS = 2
DTYPES = {"bf16": R.DTYPE_BF16, "f16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}


def _plain(**kw):
    cfg = small_config(gen_blocks=GEN_BLOCKS, **kw)
    return cfg, M.make_seeded_weights(cfg)


MODELS = {
    "default": lambda: _plain(),
    "filters3": lambda: _plain(flow_filters=(32, 64, 32)),
    "filters4_no_head": lambda: _plain(flow_filters=(32, 64, 64, 32)),
    "resnet64": lambda: _plain(flow_arch="resnet", flow_res_blocks=2, flow_res_filters=64),
    "resnet32": lambda: _plain(flow_arch="resnet", flow_res_blocks=2, flow_res_filters=32),
    "gen32": lambda: _plain(gen_filters=32),
    "lrelu": lambda: _plain(gen_activation="lrelu"),
    "brightness": lambda: _plain(normalize_brightness=True),
    "temporal": lambda: _plain(temporal_strength=0.25),
    "output_flow": lambda: M.output_flow(*_plain()),
    "flow_free": lambda: flow_free(small_config(gen_blocks=GEN_BLOCKS)),   # as test_gpu_flowfree.py builds its own
}

CASES = [(m, d, "") for m in MODELS for d in ("bf16", "f16")]
CASES += [("default", "bf16", s) for s in (
    "JU_TOWER=layers", "JU_TOWER=convs", "JU_TAIL=fused", "JU_TAIL=split", "JU_PACK=split", "JU_POOL=split",
    "JU_UPSAMPLE=split", "JU_FLOW_CONV=generic", "JU_CALIBRATE=1")]
CASES += [("resnet64", "bf16", s) for s in ("JU_FLOW=layers", "JU_FLOW=convs")]
CASES += [("default", "fp8", s) for s in ("", "JU_TOWER=layers", "JU_TOWER=convs")]


def case_id(case):
    model, dtype, switch = case
    return "%s-%s%s" % (model, dtype, "-" + switch if switch else "")


@functools.lru_cache(maxsize=None)
def blob(model):
    return M.serialize(*MODELS[model]())


@contextlib.contextmanager
def runtime(model, dtype, switch):
    """A runtime constructed under exactly `switch` (the constructor reads the switches; the environment is put back
    before anything else happens)."""
    keep = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        if switch:
            k, v = switch.split("=")
            os.environ[k] = v
        rt = R.Runtime(blob(model), 0, DTYPES[dtype])
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        yield rt
    finally:
        rt.close()


def measure(case):
    """The table of one case, in the golden file's form (JSON: lists, floats)."""
    with runtime(*case) as rt:
        got = {"stats": {k: rt.stat(k) for k in STATS}, "tags": {}}
        for tag in TAGS:
            ms, launches, flops = rt.time_steps(tag, 0)
            assert ms == 0.0
            got["tags"][tag] = [launches, flops]
        for tag in ("flow", "tower"):
            got[tag + "#k"] = [rt.time_steps("%s#%d" % (tag, k), 0)[2] for k in range(got["tags"][tag][0])]
    return got


@pytest.fixture(scope="module")
def golden():
    if os.environ.get("JU_RECORD_PROGRAM_SHAPES") == "1":
        table = {case_id(c): measure(c) for c in CASES}
        with open(GOLDEN, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_program_shape(case, golden):
    want = golden[case_id(case)]
    got = measure(case)
    print(case_id(case), json.dumps(got, sort_keys=True))
    assert got["stats"] == want["stats"]
    for tag in TAGS:
        assert got["tags"][tag] == want["tags"][tag], tag
    for tag in ("flow", "tower"):
        assert got[tag + "#k"] == want[tag + "#k"], tag
        assert sum(got[tag + "#k"]) == got["tags"][tag][1]       # (exact: integers below 2^53)
    assert sorted(got) == sorted(want)
    assert sum(n for n, _ in got["tags"].values()) == got["stats"]["launches_per_frame"]   # no tag is missing from TAGS


def test_golden_file_is_not_vacuous(golden):
    """Every form of the program appears in the file, read from the launch counts alone."""
    assert sorted(golden) == sorted(case_id(c) for c in CASES)

    def launches(cid, tag):
        return golden[cid]["tags"][tag][0]

    # the 16-bit tower: resident (one launch), per block, per convolution
    assert golden["default-bf16"]["stats"]["resident_tower"] == 1 and launches("default-bf16", "tower") == 1
    assert launches("default-bf16-JU_TOWER=layers", "tower") == GEN_BLOCKS
    assert launches("default-bf16-JU_TOWER=convs", "tower") == 2 * GEN_BLOCKS
    # the 8-bit tower: the same three, the per-block and per-convolution forms behind their quantize launch
    assert golden["default-fp8"]["stats"]["resident_tower"] == 1 and launches("default-fp8", "tower") == 1
    assert launches("default-fp8-JU_TOWER=layers", "tower") == 1 + GEN_BLOCKS
    assert launches("default-fp8-JU_TOWER=convs", "tower") == 1 + 2 * GEN_BLOCKS
    # the 16-bit resident tower runs conv_1 as its layer 0; every other tower has the head as a launch
    assert launches("default-bf16", "gen_head") == 0 and launches("default-fp8", "gen_head") == 1
    # the tail: inside the tower's launch, one fused launch, two launches
    assert launches("default-bf16", "tail") == 0
    assert launches("default-bf16-JU_TAIL=fused", "tail") == 1
    assert launches("default-bf16-JU_TAIL=split", "tail") == 2
    # the flow-resnet: resident (expand + tower + head), per block, per convolution
    assert golden["resnet64-bf16"]["stats"]["resident_flow"] == 1 and launches("resnet64-bf16", "flow") == 3
    assert launches("resnet64-bf16-JU_FLOW=layers", "flow") == 1 + 2 + 1
    assert launches("resnet64-bf16-JU_FLOW=convs", "flow") == 1 + 2 * 2 + 1
    assert golden["resnet32-bf16"]["stats"]["resident_flow"] == 0 and launches("resnet32-bf16", "flow") == 1 + 2 * 2 + 1
    # the auto-encoder: one launch per unit where planned (7 units of the default's 7 filters at most), two
    # convolutions per block and resampling launches where not
    assert launches("default-bf16", "flow") < launches("default-bf16-JU_FLOW_CONV=generic", "flow")
    assert launches("default-bf16-JU_FLOW_CONV=generic", "flow") >= 2 * 6 + 2
    # the switches that split a launch off add one (or more) to the default's count
    for s in ("JU_PACK=split", "JU_POOL=split", "JU_UPSAMPLE=split", "JU_CALIBRATE=1"):
        assert golden["default-bf16-" + s]["stats"]["launches_per_frame"] > golden["default-bf16"]["stats"]["launches_per_frame"], s
    assert launches("default-bf16-JU_PACK=split", "pack") == 1 and launches("default-bf16", "pack") == 0
    assert launches("brightness-bf16", "pack") >= 1 and launches("temporal-bf16", "temporal") == 1
    assert launches("flow_free-bf16", "lr_pack") == 1 and launches("flow_free-bf16", "flow") == 0
    assert launches("default-bf16-JU_CALIBRATE=1", "calib") == 1 + 1 + 2 * GEN_BLOCKS
