"""Which captured graph a call replays, when it captures one and when it forgets one -- needs an MI355X.

The engine keeps two caches of hipGraphs (csrc/graph_cache.h): per device frame pair and binding set, and per tuple of
frames of a look-ahead pass.  This file runs ONE fixed sequence of calls over both and records after every call

    (graph_replays, eager_runs, graph_captures, prepared_captures, registered_pairs, direct_graphs, lookahead_frames)

compared with `==` against tests/golden/graph_trace.json.  The sequence: unregistered pairs at their first, second and
third sighting; registered pairs; an unregistered and a registered 4-tuple; every selective drop (a shorter look-ahead
cap, the scene detector's mode, a stage setter), the drop of everything at the resident tower's fallback, and what a
registered pair and a formerly registered tuple do behind it.  Every frame a call writes is also compared with a second
runtime that takes the same frames one by one through ju_process under the same settings.

The golden file was recorded from the library BEFORE the two caches were written as one component
(JU_RECORD_GRAPH_TRACE=1 writes it) and is not to be recorded again from a cache that was edited since: a difference is
a finding about the cache, not about the file.
"""

import json
import os

import numpy as np
import pytest

from helpers import M, ROOT, small_config
from joshupscale_amd import runtime as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_trace.json")
STATS = ("graph_replays", "eager_runs", "graph_captures", "prepared_captures", "registered_pairs", "direct_graphs",
         "lookahead_frames")
FRAMES = 16
A, B, C, D = (4, 5, 6, 7), (8, 9, 10, 11), (12, 13, 14, 15), (0, 1, 2, 3)   # 4-tuples of input frames
OUTS = (0, 1, 2, 3)


def sequence():
    """(op, args...): `process` in-frame, out-buffer; `batch` / `prepare_batch` in-frames, out-buffers."""
    ops = []
    # 1. unregistered pairs: the key holds the binding set, which alternates -- five calls show one tuple three times
    ops += [("process", 0, 0)] * 5 + [("process", 1, 1)] * 2
    # 2. two registered pairs, then their use
    ops += [("prepare_frames", 2, 0), ("prepare_frames", 3, 0), ("prepare_frames", 2, 0)]
    ops += [("process", 2, 0), ("process", 3, 0), ("process", 2, 0), ("process", 3, 0)]
    # 3. an unregistered 4-tuple, three times
    ops += [("batch", A, OUTS)] * 3
    # 4. a registered 4-tuple, then its use
    ops += [("prepare_batch", B, OUTS), ("prepare_batch", B, OUTS), ("batch", B, OUTS), ("batch", B, OUTS)]
    # 5. a shorter cap drops the longer passes, the registered one too: the tuple goes as two passes of two, and as one
    # unregistered pass of four once the cap is back
    ops += [("set_lookahead", 2), ("batch", B, OUTS), ("set_lookahead", 8), ("batch", B, OUTS)]
    # 6. the detector around a pass: a mode change drops the graphs of the passes that carry it
    ops += [("scene_lookahead", 1), ("scene_detect", R.SCENE_REPORT), ("batch", C, OUTS), ("batch", C, OUTS), ("batch", C, OUTS),
            ("scene_detect", R.SCENE_OFF), ("batch", C, OUTS), ("scene_detect", R.SCENE_REPORT), ("batch", C, OUTS),
            ("scene_detect", R.SCENE_OFF)]
    # 7. a stage setter around a pass: it drops the graphs of the staged passes
    ops += [("stage_lookahead", 1), ("mask", 1), ("batch", D, OUTS), ("batch", D, OUTS), ("batch", D, OUTS), ("mask", 2),
            ("batch", D, OUTS), ("mask", 0), ("batch", D, OUTS), ("stage_lookahead", 0)]
    # 8. the resident tower's fallback (one faulted launch, on an unregistered pair: the hook acts on eager launches)
    ops += [("reset",), ("fault_process", 0, 4)]
    # 9. a registered pair and a formerly registered tuple behind it
    ops += [("process", 2, 0), ("process", 3, 0), ("process", 0, 0), ("batch", B, OUTS), ("batch", A, OUTS)]
    return ops


def mask_of(seed):
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 256, (37, 50, 4), dtype=np.uint8)
    kind = rng.integers(0, 3, (37, 50))
    mask[kind == 0, :3] = 255
    mask[kind == 1, :3] = 0
    return mask


def settings(rt, op):
    """The ops that change what a frame's bytes are: applied to both runtimes.  True if `op` was one."""
    if op[0] == "scene_detect":
        rt.set_scene_detect(op[1])
    elif op[0] == "mask":
        rt.set_source_mask(mask_of(op[1]) if op[1] else None)
    elif op[0] == "reset":
        rt.reset()
    else:
        return False
    return True


def run_trace():
    """[(op as text, the stats after it)] of the runtime under test; every frame checked against the frame-by-frame twin."""
    import torch
    cfg = small_config()
    h, w = cfg.frame_height, cfg.frame_width
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    frames = M.synthetic_frames(FRAMES, h, w, seed=83, kind="noise")
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames).to(dev)
    d_out = torch.zeros((5, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    d_ref = torch.zeros((2, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lib = R.load_library()
    ops = sequence()

    def faulted(rt, inp, out):   # exactly once per runtime, never in a loop
        lib.ju_debug_set(b"resident_fault", 1)
        try:
            rt.process(inp, out)
        finally:
            lib.ju_debug_set(b"resident_fault", 0)

    # the twin: the same frames under the same settings, one by one through ju_process
    want = []
    with R.Runtime(blob, 0, R.DTYPE_BF16) as ref:
        def src(t):
            return ref.device_image(d_in[t].data_ptr(), w, h)
        out, other = (ref.device_image(d_ref[k].data_ptr(), 4 * w, 4 * h) for k in range(2))
        for op in ops:
            got = []
            if settings(ref, op):
                pass
            elif op[0] == "process":
                ref.process(src(op[1]), out)
                got.append(d_ref[0].cpu().numpy())
            elif op[0] == "batch":
                for t in op[1]:
                    ref.process(src(t), out)
                    got.append(d_ref[0].cpu().numpy())
            elif op[0] == "fault_process":
                faulted(ref, src(op[1]), other)
                got.append(d_ref[1].cpu().numpy())
            want.append(got)
        assert ref.stat("fallbacks") == 1 and ref.stat("lookahead_frames") == 0

    trace = []
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        assert rt.stat("resident_tower") == 1

        def src(t):
            return rt.device_image(d_in[t].data_ptr(), w, h)

        def dst(k):
            return rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h)

        for i, op in enumerate(ops):
            wrote = []
            if settings(rt, op):
                pass
            elif op[0] == "process":
                rt.process(src(op[1]), dst(op[2]))
                wrote = [op[2]]
            elif op[0] == "fault_process":
                faulted(rt, src(op[1]), dst(op[2]))
                wrote = [op[2]]
            elif op[0] == "batch":
                rt.process_batch([src(t) for t in op[1]], [dst(k) for k in op[2]])
                wrote = list(op[2])
            elif op[0] == "prepare_frames":
                rt.prepare_frames(src(op[1]), dst(op[2]))
            elif op[0] == "prepare_batch":
                rt.prepare_batch([src(t) for t in op[1]], [dst(k) for k in op[2]])
            elif op[0] == "set_lookahead":
                rt.set_lookahead(op[1])
            elif op[0] == "scene_lookahead":
                rt.set_scene_lookahead(op[1])
            elif op[0] == "stage_lookahead":
                rt.set_stage_lookahead(op[1])
            else:
                raise AssertionError(op)
            assert len(wrote) == len(want[i])
            for k, ref_frame in zip(wrote, want[i]):
                assert np.array_equal(d_out[k].cpu().numpy(), ref_frame), (i, op, k)
            trace.append([" ".join(str(x) for x in op), [int(rt.stat(s)) for s in STATS]])
        assert rt.stat("fallbacks") == 1 and rt.stat("resident_tower") == 0
    return trace


def test_graph_trace():
    got = run_trace()
    for line in got:
        print(json.dumps(line))
    if os.environ.get("JU_RECORD_GRAPH_TRACE") == "1":
        with open(GOLDEN, "w") as f:
            json.dump({"stats": list(STATS), "trace": got}, f, indent=1)
            f.write("\n")
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["stats"] == list(STATS)
    assert got[-1][1][STATS.index("lookahead_frames")] > 0          # passes formed on this model
    for i, (g, want) in enumerate(zip(got, golden["trace"])):
        assert g == want, (i, g, want)
    assert len(got) == len(golden["trace"])
    # the file is not vacuous: every counter moved, the fallback emptied the pair cache and kept the registrations
    stats = np.array([s for _, s in golden["trace"]])
    assert (stats.max(axis=0) > 0).all()
    fault = next(i for i, (op, _) in enumerate(golden["trace"]) if op.startswith("fault_process"))
    assert stats[fault][STATS.index("direct_graphs")] == 0 and stats[fault][STATS.index("registered_pairs")] == 2
    assert stats[fault + 1][STATS.index("graph_captures")] == stats[fault][STATS.index("graph_captures")] + 1
