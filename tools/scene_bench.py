"""What the scene detector (docs/scene_detect.md) costs per frame: ju_process on device frames, psp-quality bf16
(480x270 -> 1920x1080), bench.py's clip and loop (a ring of 16 registered frame-buffer pairs, uniform noise: a clip
without cuts -- its S_t is large and constant, so D_t is small), with the mode off, JU_SCENE_REPORT and JU_SCENE_RESET.

The three runtimes live in one process and are timed in turn, --runs times over, --frames synchronous calls each after
--warmup, so that the clock and the other work on the machine are shared alike.  The comparison is the mode off in the
same build.  Prints one JSON line: frames/s of every run, their median and spread, the overhead per frame against the
mode off, and the cuts each runtime saw (0: the clip has none).

--profile N instead runs N frames of the two detecting runtimes only, for a
`rocprofv3 --kernel-trace --stats -- python tools/scene_bench.py --profile N` run of its own."""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch's HIP runtime first, as bench.py does)

from joshupscale_amd import model_file as M  # noqa: E402
from joshupscale_amd import runtime as R  # noqa: E402

RING = 16
MODES = (("off", R.SCENE_OFF), ("report", R.SCENE_REPORT), ("reset", R.SCENE_RESET))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=10000)
    ap.add_argument("--profile", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(RING, h, w, seed=1234, kind="noise")
    d_in = torch.from_numpy(clip).to(dev)
    d_out = torch.empty((RING, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    runtimes, refs = {}, {}
    for name, mode in MODES:
        rt = R.Runtime(blob, 0, R.DTYPE_BF16, hooks=False)
        if mode != R.SCENE_OFF:
            rt.set_scene_detect(mode, args.threshold)
        ins = [rt.device_image(d_in[i].data_ptr(), w, h) for i in range(RING)]
        outs = [rt.device_image(d_out[i].data_ptr(), 4 * w, 4 * h) for i in range(RING)]
        for i in range(RING):
            rt.prepare_frames(ins[i], outs[i])
        runtimes[name] = rt
        refs[name] = (ins, outs, [C.byref(x) for x in ins], [C.byref(x) for x in outs])

    def run(name, count):
        rt = runtimes[name]
        ins, outs, rin, rout = refs[name]
        proc, hnd = rt._lib.ju_process, rt._h
        for i in range(count):
            pos = i % RING
            if proc(hnd, rin[pos], rout[pos]):
                rt.process(ins[pos], outs[pos])                   # (raises with the runtime's message)

    if args.profile:
        for name in ("report", "reset"):
            run(name, args.profile)
        print(json.dumps({"profiled": ["report", "reset"], "frames_each": args.profile}))
        return
    for name, _ in MODES:
        run(name, args.warmup)
    rates = {name: [] for name, _ in MODES}
    for _ in range(args.runs):
        for name, _mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.frames)
            torch.cuda.synchronize()
            rates[name].append(args.frames / (time.perf_counter() - t0))
    us = {k: 1e6 / float(np.median(v)) for k, v in rates.items()}
    result = {"tool": "scene_bench", "preset": args.preset, "dtype": "bf16", "frames": args.frames, "runs": args.runs,
              "threshold_milli": args.threshold,
              "frames_per_s": {k: {"runs": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1),
                                   "spread_percent": round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2)}
                               for k, v in rates.items()},
              "us_per_frame": {k: round(v, 2) for k, v in us.items()},
              "overhead_us_per_frame": {k: round(us[k] - us["off"], 2) for k in ("report", "reset")},
              "scene_cuts": {k: runtimes[k].stat("scene_cuts") for k in runtimes},
              "scene_frames": {k: runtimes[k].stat("scene_frames") for k in runtimes},
              "graph_replays": {k: runtimes[k].stat("graph_replays") for k in runtimes}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
