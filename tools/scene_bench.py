"""What the scene detector (docs/scene_detect.md) costs per frame: ju_process on device frames, psp-quality bf16
(480x270 -> 1920x1080), bench.py's clip and loop (a ring of 16 registered frame-buffer pairs, uniform noise: a clip
without cuts -- its S_t is large and constant, so D_t is small), with the mode off, JU_SCENE_REPORT and JU_SCENE_RESET.

The three runtimes live in one process and are timed in turn, --runs times over, --frames synchronous calls each after
--warmup, so that the clock and the other work on the machine are shared alike.  The comparison is the mode off in the
same build.  Prints one JSON line: frames/s of every run, their median and spread, the overhead per frame against the
mode off, and the cuts each runtime saw (0: the clip has none).

--profile N instead runs N frames of the two detecting runtimes only, for a
`rocprofv3 --kernel-trace --stats -- python tools/scene_bench.py --profile N` run of its own.

--passes N (2 .. 8) is the pass mode (docs/scene_detect.md "Passes"): the same three modes, each frame by frame
(ju_process, the setting off) and in look-ahead passes of N device frames (ju_process_batch on registered tuples; with
the detector on that needs ju_set_scene_lookahead), six runtimes interleaved in one process.  --clip cuts replaces the
noise clip by four smooth scenes of four frames, so that the ring has a cut every fourth frame and JU_SCENE_RESET
really zeroes.  --tree PATH imports the package (and with it the library) from another checkout -- the parent commit's
build, for the rows that must not have moved; rows that need the setting are left out there, and --rows common leaves
them out of this build's run too, so that both processes hold the same four runtimes."""

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

if "--tree" in sys.argv:  # (before the package is imported: another checkout's)
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]))

from joshupscale_amd import model_file as M  # noqa: E402
from joshupscale_amd import runtime as R  # noqa: E402

RING = 16
MODES = (("off", R.SCENE_OFF), ("report", R.SCENE_REPORT), ("reset", R.SCENE_RESET))


def make_clip(kind, h, w):
    if kind == "noise":
        return M.synthetic_frames(RING, h, w, seed=1234, kind="noise")
    scenes = [M.synthetic_frames(4, h, w, seed=seed, kind="smooth") for seed in (1, 2, 3, 4)]
    return np.ascontiguousarray(np.concatenate(scenes, axis=0))


def pass_mode(args, blob, h, w, d_in, d_out):
    """Every mode frame by frame and in passes of args.passes frames; one JSON line."""
    n = args.passes
    tuples = [list(range(lo, lo + n)) for lo in range(0, RING - n + 1, n)]
    has_setting = hasattr(R.Runtime, "set_scene_lookahead")
    rows = {}
    for name, mode in MODES:
        for path in ("frames", "passes"):
            if path == "passes" and mode != R.SCENE_OFF and (not has_setting or args.rows == "common"):
                continue
            rt = R.Runtime(blob, 0, R.DTYPE_BF16, hooks=False)
            rt.set_lookahead(n)
            if mode != R.SCENE_OFF:
                rt.set_scene_detect(mode, args.threshold)
                if path == "passes":
                    rt.set_scene_lookahead(1)
            ins = [rt.device_image(d_in[i].data_ptr(), w, h) for i in range(RING)]
            outs = [rt.device_image(d_out[i].data_ptr(), 4 * w, 4 * h) for i in range(RING)]
            if path == "frames":
                for i in range(RING):
                    rt.prepare_frames(ins[i], outs[i])
                calls = [(C.byref(ins[i]), C.byref(outs[i])) for i in range(RING)]
            else:
                calls = []
                for t in tuples:
                    a, b = (R.JuImage * n)(*[ins[i] for i in t]), (R.JuImage * n)(*[outs[i] for i in t])
                    if rt.prepare_batch([ins[i] for i in t], [outs[i] for i in t]) != 2:
                        raise RuntimeError("the tuple was not captured as one pass: %s / %s" % (name, path))
                    calls.append((a, b))
            rows[name + "/" + path] = (rt, path, calls, (ins, outs))

    def run(key, frames):
        rt, path, calls, _keep = rows[key]
        if path == "frames":
            proc, hnd = rt._lib.ju_process, rt._h
            for i in range(frames):
                a, b = calls[i % len(calls)]
                if proc(hnd, a, b):
                    raise RuntimeError(rt._lib.ju_last_error().decode())
        else:
            proc, hnd = rt._lib.ju_process_batch, rt._h
            for i in range(frames // n):
                a, b = calls[i % len(calls)]
                if proc(hnd, a, b, n):
                    raise RuntimeError(rt._lib.ju_last_error().decode())

    frames = args.frames // n * n
    for key in rows:
        run(key, max(args.warmup // n, 2 * len(tuples)) * n)
    rates = {key: [] for key in rows}
    for _ in range(args.runs):
        for key in rows:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, frames)
            torch.cuda.synchronize()
            rates[key].append(frames / (time.perf_counter() - t0))
    us = {k: 1e6 / float(np.median(v)) for k, v in rates.items()}

    def stat(rt, key):
        try:
            return rt.stat(key)
        except R.JoshUpscaleError:
            return None
    print(json.dumps({
        "tool": "scene_bench", "mode": "passes", "pass_frames": n, "clip": args.clip, "preset": args.preset, "dtype": "bf16",
        "frames": frames, "runs": args.runs, "threshold_milli": args.threshold, "tree": args.tree or ".", "rows": args.rows,
        "frames_per_s": {k: {"runs": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1),
                             "spread_percent": round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2)}
                         for k, v in rates.items()},
        "us_per_frame": {k: round(v, 2) for k, v in us.items()},
        "scene_cuts": {k: stat(rows[k][0], "scene_cuts") for k in rows},
        "scene_frames": {k: stat(rows[k][0], "scene_frames") for k in rows},
        "lookahead_frames": {k: stat(rows[k][0], "lookahead_frames") for k in rows},
        "scene_pass_frames": {k: stat(rows[k][0], "scene_pass_frames") for k in rows},
        "graph_captures": {k: stat(rows[k][0], "graph_captures") for k in rows}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=10000)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--passes", type=int, default=0)
    ap.add_argument("--clip", choices=("noise", "cuts"), default="noise")
    ap.add_argument("--tree", default="")
    ap.add_argument("--rows", choices=("all", "common"), default="all")
    args = ap.parse_args()
    if args.passes and not 2 <= args.passes <= 8:
        ap.error("--passes takes 2 .. 8")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    clip = make_clip(args.clip, h, w)
    d_in = torch.from_numpy(clip).to(dev)
    d_out = torch.empty((RING, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if args.passes:
        return pass_mode(args, blob, h, w, d_in, d_out)
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
